// csc_abi.hip -- the extern "C" entry points of the solver handle (include/sporco_amd.h): argument
// checks, device selection, exceptions -> return codes.  All work happens behind CscBase
// (csc_impl.h; implemented by template Csc<T> in csc_api.hip).
#include "csc_impl.h"

using namespace sporco_amd;

// ---- what the entry points of every handle share (called between SA_API_BEGIN and SA_API_END) ------------------
static void require_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        throw Error(SPORCO_AMD_EHIP, "no HIP device visible: libsporco_amd needs an AMD GPU");
    SA_REQUIRE(device >= 0 && device < n, "device index out of range");
}

// a live handle, its device current
template <class H> static void check_handle(H *h) {
    SA_REQUIRE(h != nullptr && h->impl, "null handle");
    SA_HIP(hipSetDevice(h->device));
}

// a side handle (csc_impl.h SideHandle) around what make() returns; the family's own argument checks come first
template <class H, class Make> static void create_handle(int device, H **out, Make make) {
    SA_REQUIRE(out != nullptr, "null argument");
    require_device(device);
    std::unique_ptr<H> h(new H);
    h->device = device;
    h->impl.reset(make());
    *out = h.release();
}

template <class H> static void destroy_handle(H *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

template <class H> static void sync_handle(H *h) {
    check_handle(h);
    h->impl->sync();
}

// timing on / off: the stream drained by the caller's sync, what is pending folded into the totals
static void profile_enable(Profiler &pr, int enable) {
    pr.drain();
    // create the event pool up front: hipEventCreate is slow enough to distort a timed region if it happens
    // lazily inside it
    while (enable && pr.pool.size() < 512) {
        hipEvent_t e;
        SA_HIP(hipEventCreate(&e));
        pr.pool.push_back(e);
    }
    pr.on = enable != 0;
}

// one slot's name, total and launch count since the last read
static void profile_read(Profiler &pr, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_REQUIRE(slot >= 0 && slot < PS_COUNT, "timing slot out of range");
    pr.drain();
    if (name) *name = kProfNames[slot];
    if (total_ms) *total_ms = pr.total_ms[slot];
    if (launches) *launches = pr.count[slot];
    pr.total_ms[slot] = 0.0;
    pr.count[slot] = 0;
}

template <class H> static void profile_handle(H *h, int enable) {
    sync_handle(h);
    profile_enable(h->impl->prof, enable);
}

template <class H>
static void profile_read_handle(H *h, int slot, const char **name, double *total_ms, int64_t *launches) {
    check_handle(h);
    profile_read(h->impl->prof, slot, name, total_ms, launches);
}

extern "C" {

const char *sporco_amd_version(void) { return "sporco_amd 0.1.0 (gfx950)"; }
const char *sporco_amd_last_error(void) { return g_last_error.c_str(); }

int sporco_amd_device_count(int *count) {
    SA_API_BEGIN
    SA_REQUIRE(count != nullptr, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        n = 0;
        (void)hipGetLastError();
    }
    *count = n;
    SA_API_END
}

int sporco_amd_device_info(int device, char *name, size_t name_len, int *cu_count,
                           size_t *hbm_bytes) {
    SA_API_BEGIN
    hipDeviceProp_t prop;
    SA_HIP(hipGetDeviceProperties(&prop, device));
    if (name && name_len) {
        std::strncpy(name, prop.name, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    SA_API_END
}

int sporco_amd_csc_create(const sporco_amd_dims *dims, int device, void *stream,
                          sporco_amd_csc_t *out) {
    return sporco_amd_csc_create_mc(dims, 1, device, stream, out);
}

int sporco_amd_csc_create_mc(const sporco_amd_dims *dims, int32_t dict_channels, int device,
                             void *stream, sporco_amd_csc_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(dims && out, "null argument");
    SA_REQUIRE(dict_channels >= 1, "dict_channels must be >= 1");
    require_device(device);
    std::unique_ptr<sporco_amd_csc> h(new sporco_amd_csc);
    h->device = device;
    h->impl.reset(make_csc(*dims, dict_channels, device, stream));
    *out = h.release();
    SA_API_END
}

int sporco_amd_csc_create_volume(const sporco_amd_dims *dims, int32_t depth, int device, void *stream,
                                 sporco_amd_csc_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(dims && out, "null argument");
    SA_REQUIRE(depth >= 1 && dims->H % depth == 0, "depth must divide the folded first axis dims->H");
    require_device(device);
    std::unique_ptr<sporco_amd_csc> h(new sporco_amd_csc);
    h->device = device;
    h->depth = depth;
    h->impl.reset(make_csc(*dims, 1, device, stream, depth));
    *out = h.release();
    SA_API_END
}

int sporco_amd_csc_destroy(sporco_amd_csc_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_csc_sync(sporco_amd_csc_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_csc_stream(sporco_amd_csc_t h, void **stream) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(stream, "null argument");
    *stream = h->impl->stream_handle();
    SA_API_END
}

int sporco_amd_csc_set_hint(sporco_amd_csc_t h, int what, int value) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->set_hint(what, value);
    SA_API_END
}

int sporco_amd_csc_query(sporco_amd_csc_t h, int what, int *out) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "null output pointer");
    *out = h->impl->query(what);
    SA_API_END
}

int sporco_amd_csc_placement_report(sporco_amd_csc_t h, char *buf, size_t cap) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(buf != nullptr && cap > 0, "null or empty report buffer");
    const std::string r = h->impl->placement();
    std::snprintf(buf, cap, "%s", r.c_str());
    SA_API_END
}

int sporco_amd_csc_set_signal(sporco_amd_csc_t h, const void *S) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(S != nullptr, "S is null");
    h->impl->set_signal(S);
    SA_API_END
}

int sporco_amd_csc_set_dict(sporco_amd_csc_t h, const void *D, int32_t dH, int32_t dW) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(D != nullptr, "D is null");
    h->impl->set_dict(D, dH, dW);
    SA_API_END
}

int sporco_amd_csc_set_dict_imag(sporco_amd_csc_t h, const void *D_imag, int32_t dH, int32_t dW) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->set_dict_imag(D_imag, dH, dW);
    SA_API_END
}

int sporco_amd_csc_set_l1_weight(sporco_amd_csc_t h, const void *w, const int64_t shape[5]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(w == nullptr || shape != nullptr, "shape is null");
    h->impl->set_weight(0, w, shape);
    SA_API_END
}

int sporco_amd_csc_set_l21_weight(sporco_amd_csc_t h, const void *w, const int64_t shape[5]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(w == nullptr || shape != nullptr, "shape is null");
    h->impl->set_weight(1, w, shape);
    SA_API_END
}

int sporco_amd_csc_set_ams_mask(sporco_amd_csc_t h, const void *w, const int64_t shape[5]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(w == nullptr || shape != nullptr, "shape is null");
    h->impl->set_weight(2, w, shape);
    SA_API_END
}

int sporco_amd_csc_set_grad_weight(sporco_amd_csc_t h, const void *w) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->set_grad_weight(w);
    SA_API_END
}

int sporco_amd_csc_set_filter_sizes(sporco_amd_csc_t h, const int32_t *fh, const int32_t *fw) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE((fh == nullptr) == (fw == nullptr), "both size arrays, or neither");
    h->impl->set_filter_sizes(fh, fw);
    SA_API_END
}

int sporco_amd_csc_upload(sporco_amd_csc_t h, int var, const void *src) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(src != nullptr, "src is null");
    h->impl->upload(var, src);
    SA_API_END
}

int sporco_amd_csc_download(sporco_amd_csc_t h, int var, void *dst) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(dst != nullptr, "dst is null");
    h->impl->download(var, dst);
    SA_API_END
}

int sporco_amd_csc_device_ptr(sporco_amd_csc_t h, int var, void **ptr_dev) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(ptr_dev != nullptr, "ptr_dev is null");
    *ptr_dev = h->impl->device_ptr(var);
    SA_API_END
}

int sporco_amd_csc_admm_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && out, "null argument");
    h->impl->admm_iter(*p, h->impl->out_dev_default);
    h->impl->read_out(h->impl->out_dev_default, out);
    SA_API_END
}

int sporco_amd_csc_admm_run(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            const sporco_amd_admm_ctrl *c, sporco_amd_admm_record *records,
                            int32_t *n_done, double *rho_out, double *u_scale_out,
                            sporco_amd_reduce_fn reduce, void *user) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && c && records && n_done && rho_out && u_scale_out, "null argument");
    const int n = h->impl->admm_run(*p, *c, records, rho_out, u_scale_out, reduce, user);
    if (n < 0) {
        *n_done = 0;
        return SPORCO_AMD_EUNSUPPORTED;
    }
    *n_done = n;
    SA_API_END
}

int sporco_amd_csc_admm_iter_dev(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                                 double *out_dev) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && out_dev, "null argument");
    h->impl->admm_iter(*p, out_dev);
    SA_API_END
}

int sporco_amd_csc_admm_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && out, "null argument");
    h->impl->admm_xstep(*p, h->impl->out_dev_default);
    h->impl->read_out(h->impl->out_dev_default, out);
    SA_API_END
}

int sporco_amd_csc_admm_relax(sporco_amd_csc_t h, double rlx) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->admm_relax(rlx);
    SA_API_END
}

int sporco_amd_csc_admm_ystep(sporco_amd_csc_t h, const sporco_amd_admm_params *p) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p, "null argument");
    h->impl->admm_ystep(*p);
    SA_API_END
}

int sporco_amd_csc_admm_ustep(sporco_amd_csc_t h, const sporco_amd_admm_params *p) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p, "null argument");
    h->impl->admm_ustep(*p);
    SA_API_END
}

int sporco_amd_csc_admm_stats(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && out, "null argument");
    h->impl->admm_stats(*p, h->impl->out_dev_default);
    h->impl->read_out(h->impl->out_dev_default, out);
    SA_API_END
}

int sporco_amd_csc_scale_u(sporco_amd_csc_t h, double s) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->scale_u(s);
    SA_API_END
}

int sporco_amd_csc_reconstruct(sporco_amd_csc_t h, int var, void *dst) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(dst != nullptr, "dst is null");
    h->impl->reconstruct(var, dst);
    SA_API_END
}

int sporco_amd_csc_dhs_absmax(sporco_amd_csc_t h, double *out) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    h->impl->dhs_absmax(out);
    SA_API_END
}

static double *stats_buf(sporco_amd_csc_t h) {
    if (!h->stats_dev) {
        SA_HIP(hipMalloc((void **)&h->stats_dev, sizeof(double) * kOutSlots));
        SA_HIP(hipMemset(h->stats_dev, 0, sizeof(double) * kOutSlots));
    }
    return h->stats_dev;
}

int sporco_amd_csc_pgm_grad(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->pgm_grad(var, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_pgm_commit(sporco_amd_csc_t h) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->pgm_commit();
    SA_API_END
}
int sporco_amd_csc_pgm_iter(sporco_amd_csc_t h, const sporco_amd_pgm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->pgm_iter(*p, stats_buf(h));
    h->impl->read_out(stats_buf(h), out);
    SA_API_END
}

int sporco_amd_csc_pgm_eval(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->pgm_eval(var, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_pgm_prox_step(sporco_amd_csc_t h, double L, double lmbda, uint32_t flags,
                                 int32_t dH, int32_t dW, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(L > 0.0, "L must be positive");
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->pgm_prox_step(L, lmbda, flags, dH, dW, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_lincomb(sporco_amd_csc_t h, int dst, double a, int va, double b, int vb,
                           double c, int vc) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->lincomb(dst, a, va, b, vb, c, vc);
    SA_API_END
}

int sporco_amd_csc_pair_stats(sporco_amd_csc_t h, int va, int vb, int vg,
                              double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->pair_stats(va, vb, vg, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_pgm_resid(sporco_amd_csc_t h, int var, int slot) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->pgm_resid(var, slot);
    SA_API_END
}

int sporco_amd_csc_pgm_resid_stats(sporco_amd_csc_t h, int a, int b, int c, int d,
                                   double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->pgm_resid_stats(a, b, c, d, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_fft_var(sporco_amd_csc_t h, int real_var, int cplx_var) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->fft_var(real_var, cplx_var, false);
    SA_API_END
}

int sporco_amd_csc_ifft_var(sporco_amd_csc_t h, int cplx_var, int real_var) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->fft_var(real_var, cplx_var, true);
    SA_API_END
}

int sporco_amd_csc_copy(sporco_amd_csc_t h, int dst_var, int src_var) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->copy(dst_var, src_var);
    SA_API_END
}

int sporco_amd_csc_ccmod_setcoef(sporco_amd_csc_t h, int var) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->ccmod_setcoef(var);
    SA_API_END
}

int sporco_amd_csc_ccmod_grad(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->ccmod_grad(var, true, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_ccmod_eval(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->ccmod_grad(var, false, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_ccmod_prox_step(sporco_amd_csc_t h, double L, int32_t dH, int32_t dW,
                                   int32_t zero_mean) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(L > 0.0, "L must be positive");
    h->impl->ccmod_prox_step(L, dH, dW, zero_mean != 0);
    SA_API_END
}

int sporco_amd_csc_ccmod_cnstr(sporco_amd_csc_t h, int32_t dH, int32_t dW, int32_t zero_mean,
                               double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->ccmod_cnstr(dH, dW, zero_mean != 0, sb);
    h->impl->read_out(sb, out);
    out[0] = std::sqrt(out[0]);
    SA_API_END
}

int sporco_amd_csc_ccmod_getdict(sporco_amd_csc_t h, int32_t dH, int32_t dW, void *dst) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(dst != nullptr, "dst is null");
    h->impl->ccmod_getdict(dH, dW, dst);
    SA_API_END
}

int sporco_amd_csc_setdict_from_dstep(sporco_amd_csc_t h, int32_t dH, int32_t dW) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->setdict_from_dstep(dH, dW);
    SA_API_END
}

int sporco_amd_csc_set_data_mask(sporco_amd_csc_t h, const void *w, const int64_t shape[5]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(w == nullptr || shape != nullptr, "shape is null");
    h->impl->set_weight(3, w, shape);
    SA_API_END
}

int sporco_amd_csc_masked_grad(sporco_amd_csc_t h, int var, int32_t dstep, int32_t write_grad,
                               double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->masked_grad(var, dstep != 0, write_grad, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_cns_init(sporco_amd_csc_t h, const void *Y0, double rho) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    h->impl->cns_init(Y0, rho);
    SA_API_END
}

int sporco_amd_csc_cns_mean_ptr(sporco_amd_csc_t h, void **ptr_dev, int64_t *count) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(ptr_dev && count, "null argument");
    *ptr_dev = h->impl->cns_mean_ptr(count);
    SA_API_END
}

int sporco_amd_csc_cns_md_init(sporco_amd_csc_t h, const void *S) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->cns_md_init(S);
    SA_API_END
}

int sporco_amd_csc_cns_iter(sporco_amd_csc_t h, const sporco_amd_cns_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->cns_iter(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_ccmod_sgd_step(sporco_amd_csc_t h, double eta, int32_t dH, int32_t dW,
                                  int32_t zero_mean, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->ccmod_sgd_step(eta, dH, dW, zero_mean != 0, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_mdcpl_init(sporco_amd_csc_t h, const void *S) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->mdcpl_init(S);
    SA_API_END
}

int sporco_amd_csc_mdcpl_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->mdcpl_iter(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_l1l1_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->l1l1_iter(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_ball_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->ball_iter(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_projl1_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p, double gamma,
                               double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(p && out, "null argument");
    h->impl->projl1_iter(*p, gamma, stats_buf(h), out);
    SA_API_END
}

int sporco_amd_csc_inhib_setup(sporco_amd_csc_t h, const double *Wg, int32_t Ng,
                               const double *taps_rows, int32_t ntaps_rows, const double *taps_cols,
                               int32_t ntaps_cols, int32_t want_self, double lmbda) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(taps_rows && taps_cols, "null taps");
    h->impl->inhib_setup(Wg, Ng, taps_rows, ntaps_rows, taps_cols, ntaps_cols, want_self != 0, lmbda);
    SA_API_END
}

int sporco_amd_csc_inhib_update(sporco_amd_csc_t h, const sporco_amd_inhib_params *p,
                                double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->inhib_update(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_tv_setup(sporco_amd_csc_t h, const double *tvw, int32_t n, int32_t vector_tv) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(tvw != nullptr, "null TVWeight");
    h->impl->tv_setup(tvw, n, vector_tv != 0);
    SA_API_END
}

int sporco_amd_csc_tv_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->tv_xstep(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_tv_ystep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->tv_ystep(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_tv_adjoint(sporco_amd_csc_t h, double u_scale, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(out, "null argument");
    double *dev = stats_buf(h);
    h->impl->tv_adjoint(u_scale, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_rtv_setup(sporco_amd_csc_t h, const double *tvw, int32_t n) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(tvw != nullptr, "null TVWeight");
    h->impl->rtv_setup(tvw, n);
    SA_API_END
}

int sporco_amd_csc_rtv_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->rtv_xstep(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_rtv_ystep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->rtv_ystep(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_rtv_dual(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->rtv_dual(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_pd_setup(sporco_amd_csc_t h, const double *B, const double *Q, const double *gamma,
                            const void *S, int32_t cs) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(B && Q && gamma && S, "null argument");
    h->impl->pd_setup(B, Q, gamma, S, cs);
    SA_API_END
}

int sporco_amd_csc_pdl1_setup(sporco_amd_csc_t h, const double *B, const double *Q, const double *gamma,
                              const void *S, int32_t cs, const void *mask) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(B && Q && gamma && S, "null argument");
    h->impl->pdl1_setup(B, Q, gamma, S, cs, mask);
    SA_API_END
}

int sporco_amd_csc_pdl1_block0(sporco_amd_csc_t h, int32_t which, int32_t upload, void *buf) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(buf, "null argument");
    h->impl->pdl1_block0(which, upload != 0, buf);
    SA_API_END
}

int sporco_amd_csc_pdl1_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->pdl1_iter(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_pd_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->pd_xstep(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_pd_dfid(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(out != nullptr, "null argument");
    double *dev = stats_buf(h);
    h->impl->pd_dfid(var, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_pd_reconstruct(sporco_amd_csc_t h, int var, void *out) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->pd_reconstruct(var, out);
    SA_API_END
}

int sporco_amd_csc_dstep_init(sporco_amd_csc_t h, const void *Y0) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->dstep_init(Y0);
    SA_API_END
}

int sporco_amd_csc_dstep_md_init(sporco_amd_csc_t h, const void *Y0, const void *S) {
    SA_API_BEGIN
    SA_HANDLE(h);
    h->impl->dstep_md_init(Y0, S);
    SA_API_END
}

int sporco_amd_csc_dstep_iter(sporco_amd_csc_t h, const sporco_amd_dstep_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE(h);
    SA_REQUIRE(p && out, "null argument");
    double *dev = stats_buf(h);
    h->impl->dstep_iter(*p, dev);
    h->impl->read_out(dev, out);
    SA_API_END
}

int sporco_amd_csc_asum(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    SA_HANDLE_ANY(h);
    SA_REQUIRE(out != nullptr, "out is null");
    double *sb = stats_buf(h);
    h->impl->asum(var, sb);
    h->impl->read_out(sb, out);
    SA_API_END
}

int sporco_amd_csc_profile(sporco_amd_csc_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_profile_slots(void) { return PS_COUNT; }

int sporco_amd_csc_profile_read(sporco_amd_csc_t h, int slot, const char **name, double *total_ms,
                                int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

// ---- TVL2Denoise: a side handle (csc_impl.h TvdBase) ----------------------------------------

int sporco_amd_tvd_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int device,
                          void *stream, sporco_amd_tvd_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(H >= 2 && W >= 2 && P >= 1 && C >= 1, "tvd: H, W >= 2, P, C >= 1");
    create_handle(device, out, [&] { return make_tvd(dtype, H, W, P, C, vector_tv != 0, false, device, stream); });
    SA_API_END
}

int sporco_amd_tvl1_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int device,
                           void *stream, sporco_amd_tvd_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(H >= 2 && W >= 2 && P >= 1 && C >= 1, "tvl1: H, W >= 2, P, C >= 1");
    create_handle(device, out, [&] { return make_tvd(dtype, H, W, P, C, vector_tv != 0, true, device, stream); });
    SA_API_END
}

int sporco_amd_tvd_destroy(sporco_amd_tvd_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_tvd_sync(sporco_amd_tvd_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_tvd_plan(sporco_amd_tvd_t h, int64_t out[6]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->plan(out);
    SA_API_END
}

int sporco_amd_tvd_upload(sporco_amd_tvd_t h, int var, const void *src, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->upload(var, src, on_device != 0);
    SA_API_END
}

int sporco_amd_tvd_download(sporco_amd_tvd_t h, int var, void *dst, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->download(var, dst, on_device != 0);
    SA_API_END
}

int sporco_amd_tvd_sweeps(sporco_amd_tvd_t h, const sporco_amd_tvd_params *p, int32_t n) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && n >= 0, "bad argument");
    h->impl->sweeps(*p, n);
    SA_API_END
}

int sporco_amd_tvd_gsres(sporco_amd_tvd_t h, const sporco_amd_tvd_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->gsres(*p, out);
    SA_API_END
}

int sporco_amd_tvd_ystep(sporco_amd_tvd_t h, const sporco_amd_tvd_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->ystep(*p, out);
    SA_API_END
}

int sporco_amd_tvd_adjoint(sporco_amd_tvd_t h) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->adjoint();
    SA_API_END
}

int sporco_amd_tvd_profile(sporco_amd_tvd_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_tvd_profile_read(sporco_amd_tvd_t h, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

// ---- TVL2Deconv / TVL1Deconv: a side handle (csc_impl.h TvdcBase) ---------------------------------

static int tvdc_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int64_t PA, bool l1,
                       int device, void *stream, sporco_amd_tvdc_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(H >= 2 && W >= 2 && P >= 1 && C >= 1, "tvdc: H, W >= 2, P, C >= 1");
    SA_REQUIRE(PA == P || PA == 1, "tvdc: the kernel has P planes or one");
    create_handle(device, out, [&] { return make_tvdc(dtype, H, W, P, C, vector_tv != 0, l1, PA, device, stream); });
    SA_API_END
}

int sporco_amd_tvdc_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int64_t PA,
                           int device, void *stream, sporco_amd_tvdc_t *out) {
    return tvdc_create(dtype, H, W, P, C, vector_tv, PA, false, device, stream, out);
}

int sporco_amd_tvl1dc_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int64_t PA,
                             int device, void *stream, sporco_amd_tvdc_t *out) {
    return tvdc_create(dtype, H, W, P, C, vector_tv, PA, true, device, stream, out);
}

int sporco_amd_tvdc_destroy(sporco_amd_tvdc_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_tvdc_sync(sporco_amd_tvdc_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_tvdc_plan(sporco_amd_tvdc_t h, int64_t out[8]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->plan(out);
    SA_API_END
}

int sporco_amd_tvdc_upload(sporco_amd_tvdc_t h, int var, const void *src, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->upload(var, src, on_device != 0);
    SA_API_END
}

int sporco_amd_tvdc_download(sporco_amd_tvdc_t h, int var, void *dst, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->download(var, dst, on_device != 0);
    SA_API_END
}

int sporco_amd_tvdc_set_kernel(sporco_amd_tvdc_t h, const void *A, int32_t ah, int32_t aw, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_kernel(A, ah, aw, on_device != 0);
    SA_API_END
}

int sporco_amd_tvdc_xstep(sporco_amd_tvdc_t h, const sporco_amd_tvdc_params *p) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr, "null argument");
    h->impl->xstep(*p);
    SA_API_END
}

int sporco_amd_tvdc_ystep(sporco_amd_tvdc_t h, const sporco_amd_tvdc_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->ystep(*p, out);
    SA_API_END
}

int sporco_amd_tvdc_adjoint(sporco_amd_tvdc_t h) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->adjoint();
    SA_API_END
}

int sporco_amd_tvdc_profile(sporco_amd_tvdc_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_tvdc_profile_read(sporco_amd_tvdc_t h, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

// ---- SplineL1: a side handle (csc_impl.h SplBase), and the stateless DCT ----------------------------

int sporco_amd_spl_create(int dtype, int32_t H, int32_t W, int64_t P, int device, void *stream, sporco_amd_spl_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(H >= 1 && W >= 2 && P >= 1, "spline: H >= 1, W >= 2, P >= 1");
    create_handle(device, out, [&] { return make_spl(dtype, H, W, P, device, stream); });
    SA_API_END
}

int sporco_amd_spl_destroy(sporco_amd_spl_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_spl_sync(sporco_amd_spl_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_spl_plan(sporco_amd_spl_t h, int64_t out[4]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->plan(out);
    SA_API_END
}

int sporco_amd_spl_upload(sporco_amd_spl_t h, int var, const void *src, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->upload(var, src, on_device != 0);
    SA_API_END
}

int sporco_amd_spl_download(sporco_amd_spl_t h, int var, void *dst, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->download(var, dst, on_device != 0);
    SA_API_END
}

int sporco_amd_spl_xstep(sporco_amd_spl_t h, const sporco_amd_spl_params *p) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr, "null argument");
    h->impl->xstep(*p);
    SA_API_END
}

int sporco_amd_spl_ystep(sporco_amd_spl_t h, const sporco_amd_spl_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->ystep(*p, out);
    SA_API_END
}

int sporco_amd_spl_profile(sporco_amd_spl_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_spl_profile_read(sporco_amd_spl_t h, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

static int spl_dct_api(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out, bool inverse, int on_device) {
    SA_API_BEGIN
    SA_REQUIRE(in && out && in != out && H >= 1 && W >= 2 && P >= 1, "dctii: bad argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        throw Error(SPORCO_AMD_EHIP, "no HIP device visible: libsporco_amd needs an AMD GPU");
    spl_dct_dispatch(dtype, H, W, P, in, out, inverse, on_device != 0);
    SA_API_END
}

int sporco_amd_dctii(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out, int on_device) {
    return spl_dct_api(dtype, H, W, P, in, out, false, on_device);
}

int sporco_amd_idctii(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out, int on_device) {
    return spl_dct_api(dtype, H, W, P, in, out, true, on_device);
}

// ---- BPDN / BPDNJoint / ElasticNet: a side handle (csc_impl.h BpdnBase) ------------------------------

int sporco_amd_bpdn_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream, sporco_amd_bpdn_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(N >= 1 && M >= 1 && K >= 1, "bpdn: N >= 1, M >= 1, K >= 1");
    SA_REQUIRE(N <= SPORCO_AMD_BPDN_MAX_DIM && M <= SPORCO_AMD_BPDN_MAX_DIM,
               "bpdn: the kernels serve dictionaries of up to 512 rows and 512 columns");
    SA_REQUIRE(K < ((int64_t)1 << 31), "bpdn: fewer than 2^31 signals");
    create_handle(device, out, [&] { return make_bpdn(dtype, N, M, K, device, stream); });
    SA_API_END
}

int sporco_amd_bpdn_destroy(sporco_amd_bpdn_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_bpdn_sync(sporco_amd_bpdn_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_bpdn_plan(sporco_amd_bpdn_t h, int64_t out[4]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->plan(out);
    SA_API_END
}

int sporco_amd_bpdn_set_dict(sporco_amd_bpdn_t h, const void *D) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_dict(D);
    SA_API_END
}

int sporco_amd_bpdn_set_solve(sporco_amd_bpdn_t h, const void *P) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_solve(P);
    SA_API_END
}

int sporco_amd_bpdn_upload(sporco_amd_bpdn_t h, int var, const void *src) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->upload(var, src);
    SA_API_END
}

int sporco_amd_bpdn_download(sporco_amd_bpdn_t h, int var, void *dst) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->download(var, dst);
    SA_API_END
}

int sporco_amd_bpdn_iter(sporco_amd_bpdn_t h, const sporco_amd_bpdn_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->iter(*p, out);
    SA_API_END
}

int sporco_amd_bpdn_profile(sporco_amd_bpdn_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_bpdn_profile_read(sporco_amd_bpdn_t h, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

int sporco_amd_bpdn_devptr(sporco_amd_bpdn_t h, int var, void **out) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    *out = h->impl->var_ptr(var);
    SA_API_END
}

// ---- pgm.bpdn BPDN / WeightedBPDN: a bpdn handle with the arrays of the proximal gradient iteration --------------
int sporco_amd_bpdn_pgm_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream, sporco_amd_bpdn_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(N >= 1 && M >= 1 && K >= 1, "bpdn: N >= 1, M >= 1, K >= 1");
    SA_REQUIRE(N <= SPORCO_AMD_BPDN_MAX_DIM && M <= SPORCO_AMD_BPDN_MAX_DIM,
               "bpdn: the kernels serve dictionaries of up to 512 rows and 512 columns");
    SA_REQUIRE(K < ((int64_t)1 << 31), "bpdn: fewer than 2^31 signals");
    create_handle(device, out, [&] { return make_pgm_bpdn(dtype, N, M, K, device, stream); });
    SA_API_END
}

int sporco_amd_bpdn_pgm_step(sporco_amd_bpdn_t h, const sporco_amd_bpdn_pgm_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr, "null argument");
    h->impl->pgm_step(*p, out);
    SA_API_END
}

int sporco_amd_bpdn_pgm_ystep(sporco_amd_bpdn_t h, double beta, double gamma, int use_zz, int advance_y,
                              double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->pgm_ystep(beta, gamma, use_zz, advance_y, out);
    SA_API_END
}

int sporco_amd_bpdn_pgm_copy(sporco_amd_bpdn_t h, int dst, int src) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->pgm_copy(dst, src);
    SA_API_END
}

// ---- CnstrMOD: a side handle (csc_impl.h CmodBase) ----------------------------------------------------

int sporco_amd_cmod_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream, sporco_amd_cmod_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(N >= 1 && M >= 1 && K >= 1, "cmod: N >= 1, M >= 1, K >= 1");
    static_assert(SPORCO_AMD_CMOD_MAX_DIM == kCmodMaxDim, "one limit for the cmod handle");
    SA_REQUIRE(N <= SPORCO_AMD_CMOD_MAX_DIM && M <= SPORCO_AMD_CMOD_MAX_DIM,
               "cmod: the kernels serve dictionaries of up to 512 rows and 512 columns");
    SA_REQUIRE(K < ((int64_t)1 << 31), "cmod: fewer than 2^31 signals");
    create_handle(device, out, [&] { return make_cmod(dtype, N, M, K, device, stream); });
    SA_API_END
}

int sporco_amd_cmod_destroy(sporco_amd_cmod_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_cmod_sync(sporco_amd_cmod_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_cmod_plan(sporco_amd_cmod_t h, int64_t out[8]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->plan(out);
    SA_API_END
}

int sporco_amd_cmod_set_signal(sporco_amd_cmod_t h, const void *S, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_signal(S, on_device != 0);
    SA_API_END
}

int sporco_amd_cmod_set_coef(sporco_amd_cmod_t h, const void *Z, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_coef(Z, on_device != 0);
    SA_API_END
}

int sporco_amd_cmod_set_solve(sporco_amd_cmod_t h, const void *Q) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_solve(Q);
    SA_API_END
}

int sporco_amd_cmod_upload(sporco_amd_cmod_t h, int var, const void *src) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->upload(var, src);
    SA_API_END
}

int sporco_amd_cmod_download(sporco_amd_cmod_t h, int var, void *dst) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->download(var, dst);
    SA_API_END
}

int sporco_amd_cmod_iter(sporco_amd_cmod_t h, const sporco_amd_cmod_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->iter(*p, out);
    SA_API_END
}

int sporco_amd_cmod_dfid(sporco_amd_cmod_t h, int var, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->dfid(var, out);
    SA_API_END
}

// ---- pgm.cmod CnstrMOD / WeightedCnstrMOD: a cmod handle with the arrays of the proximal gradient iteration ---------
int sporco_amd_cmod_pgm_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream, sporco_amd_cmod_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(N >= 1 && M >= 1 && K >= 1, "cmod: N >= 1, M >= 1, K >= 1");
    SA_REQUIRE(N <= SPORCO_AMD_CMOD_MAX_DIM && M <= SPORCO_AMD_CMOD_MAX_DIM,
               "cmod: the kernels serve dictionaries of up to 512 rows and 512 columns");
    SA_REQUIRE(K < ((int64_t)1 << 31), "cmod: fewer than 2^31 signals");
    create_handle(device, out, [&] { return make_pgm_cmod(dtype, N, M, K, device, stream); });
    SA_API_END
}

int sporco_amd_cmod_pgm_set_weight(sporco_amd_cmod_t h, const void *W, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_weight(W, on_device != 0);
    SA_API_END
}

int sporco_amd_cmod_pgm_step(sporco_amd_cmod_t h, const sporco_amd_cmod_pgm_params *p, double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr, "null argument");
    h->impl->pgm_step(*p, out);
    SA_API_END
}

int sporco_amd_cmod_profile(sporco_amd_cmod_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_cmod_profile_read(sporco_amd_cmod_t h, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

// ---- RobustPCA / prox_nuclear: a side handle (csc_impl.h RpcaBase) --------------------------------------

int sporco_amd_rpca_create(int dtype, int32_t R, int32_t C, int device, void *stream, sporco_amd_rpca_t *out) {
    SA_API_BEGIN
    SA_REQUIRE(R >= 1 && C >= 1, "rpca: R >= 1, C >= 1");
    static_assert(SPORCO_AMD_RPCA_MAX_DIM == kRpcaMaxDim, "one limit for the rpca handle");
    SA_REQUIRE((R < C ? R : C) <= SPORCO_AMD_RPCA_MAX_DIM, "rpca: the kernels serve arrays whose short side is at most 512");
    SA_REQUIRE((int64_t)R * C < ((int64_t)1 << 31), "rpca: fewer than 2^31 elements");
    create_handle(device, out, [&] { return make_rpca(dtype, R, C, device, stream); });
    SA_API_END
}

int sporco_amd_rpca_destroy(sporco_amd_rpca_t h) {
    SA_API_BEGIN
    destroy_handle(h);
    SA_API_END
}

int sporco_amd_rpca_sync(sporco_amd_rpca_t h) {
    SA_API_BEGIN
    sync_handle(h);
    SA_API_END
}

int sporco_amd_rpca_plan(sporco_amd_rpca_t h, int64_t out[10]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    h->impl->plan(out);
    SA_API_END
}

int sporco_amd_rpca_set_signal(sporco_amd_rpca_t h, const void *S, int on_device) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->set_signal(S, on_device != 0);
    SA_API_END
}

int sporco_amd_rpca_upload(sporco_amd_rpca_t h, int var, const void *src) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->upload(var, src);
    SA_API_END
}

int sporco_amd_rpca_download(sporco_amd_rpca_t h, int var, void *dst) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->download(var, dst);
    SA_API_END
}

int sporco_amd_rpca_devptr(sporco_amd_rpca_t h, int var, void **out) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(out != nullptr, "null argument");
    *out = h->impl->var_ptr(var);
    SA_API_END
}

int sporco_amd_rpca_gram(sporco_amd_rpca_t h, int mode, double u_scale, double *G) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->gram(mode, u_scale, G);
    SA_API_END
}

int sporco_amd_rpca_iter(sporco_amd_rpca_t h, const sporco_amd_rpca_params *p, const double *T,
                         double out[SPORCO_AMD_OUT_COUNT]) {
    SA_API_BEGIN
    check_handle(h);
    SA_REQUIRE(p != nullptr && out != nullptr, "null argument");
    h->impl->iter(*p, T, out);
    SA_API_END
}

int sporco_amd_rpca_apply(sporco_amd_rpca_t h, const double *T) {
    SA_API_BEGIN
    check_handle(h);
    h->impl->apply(T);
    SA_API_END
}

int sporco_amd_rpca_profile(sporco_amd_rpca_t h, int enable) {
    SA_API_BEGIN
    profile_handle(h, enable);
    SA_API_END
}

int sporco_amd_rpca_profile_read(sporco_amd_rpca_t h, int slot, const char **name, double *total_ms, int64_t *launches) {
    SA_API_BEGIN
    profile_read_handle(h, slot, name, total_ms, launches);
    SA_API_END
}

}  // extern "C"
