// api_pgm_bpdn.inc -- the handle of pgm.bpdn BPDN / WeightedBPDN (sporco/pgm/bpdn.py:26-375); kernels:
// csc_pgm_bpdn.h.  Included by csc_api.hip at namespace scope, after api_bpdn.inc: the handle is Bpdn<T> with the
// arrays of the proximal gradient iteration added, so S, the k-major zero-padded copies of D, D^T S, the stream,
// the uploads and downloads and the profile slots are that handle's.  Its arrays x / u serve as the two X arrays
// (the iterate and the one before it; a step may start by swapping their roles), y and y2 as the two Y arrays.
template <typename T> struct PgmBpdn : Bpdn<T> {
    using B = Bpdn<T>;
    int cx = 0, cy = 0;            // which X array holds the iterate, which Y array the Y in use
    T *y2 = nullptr, *g = nullptr, *zv = nullptr, *zz = nullptr, *w = nullptr;
    bool have_w = false;
    double *part_pgm = nullptr, *part_y = nullptr;

    PgmBpdn(int N_, int M_, int64_t K_, int dev, void *stream) : B(N_, M_, K_, dev, stream) {
        part_pgm = this->template dev_alloc<double>((size_t)kPgmBpdnSums * this->nb, false);
        part_y = this->template dev_alloc<double>(kBpdnMaxBlocks, false);
    }

    void plan(int64_t out[4]) override {
        B::plan(out);
        out[3] = (int64_t)pgm_bpdn_lds_bytes<T>(this->M, this->N);
    }
    void set_solve(const void *) override { throw Error(SPORCO_AMD_EINVAL, "bpdn: a pgm handle has no solve matrix"); }
    void iter(const sporco_amd_bpdn_params &, double *) override {
        throw Error(SPORCO_AMD_EINVAL, "bpdn: a pgm handle steps by sporco_amd_bpdn_pgm_step");
    }

    T *xbuf(int which) { return which == 0 ? this->x : this->u; }
    T *ybuf(int which) {
        if (which == 1) this->need(&y2);
        return which == 0 ? this->y : y2;
    }
    T *var_buf(int var) override {
        switch (var) {
        case SPORCO_AMD_BPDN_S: return this->s;
        case SPORCO_AMD_BPDN_X: return xbuf(cx);
        case SPORCO_AMD_BPDN_XPRV: return xbuf(cx ^ 1);
        case SPORCO_AMD_BPDN_Y: return ybuf(cy);
        case SPORCO_AMD_BPDN_YPRV: return ybuf(cy ^ 1);
        case SPORCO_AMD_BPDN_WL1: return this->wl1;
        case SPORCO_AMD_BPDN_DTS: return this->dts;
        case SPORCO_AMD_BPDN_G: this->need(&g); return g;
        case SPORCO_AMD_BPDN_Z: this->need(&zv); return zv;
        case SPORCO_AMD_BPDN_ZZ: this->need(&zz); return zz;
        case SPORCO_AMD_BPDN_W: return w;
        default: throw Error(SPORCO_AMD_EINVAL, "bpdn: unknown array id");
        }
    }
    size_t var_bytes(int var) const override {
        return sizeof(T) * (size_t)((var == SPORCO_AMD_BPDN_S || var == SPORCO_AMD_BPDN_W) ? this->N : this->M) * this->K;
    }
    void upload(int var, const void *src) override {
        if (var == SPORCO_AMD_BPDN_W) {
            have_w = src != nullptr;
            if (!have_w) return;
            if (!w) w = this->template dev_alloc<T>((size_t)this->N * this->K, false);
        }
        B::upload(var, src);
    }

    bool mk_var(int var) const { return var != SPORCO_AMD_BPDN_S && var != SPORCO_AMD_BPDN_W; }
    void pgm_copy(int dst, int src) override {
        SA_REQUIRE(mk_var(dst) && mk_var(src), "bpdn: copies are between (M, K) arrays");
        T *d = var_buf(dst), *s_ = var_buf(src);
        SA_REQUIRE(d != nullptr && s_ != nullptr, "bpdn: the weight is a scalar");
        if (d != s_) SA_HIP(hipMemcpyAsync(d, s_, var_bytes(dst), hipMemcpyDeviceToDevice, this->st));
    }

    void finalize_read(const double *part, int nblk, int stride, int nvals, const int *slots, const double *scales,
                       double *out_host) {
        {
            ProfScope ps(this->prof, PS_FINALIZE);
            launch_finalize(this->st, part, nblk, stride, nvals, slots, scales, false, this->out_dev);
        }
        if (out_host) this->read_out(out_host);
    }

    void pgm_step(const sporco_amd_bpdn_pgm_params &p, double *out_host) override {
        SA_REQUIRE(this->have_s && this->have_d, "bpdn: S and the dictionary are set before the first step");
        SA_REQUIRE(p.L > 0.0, "L must be positive");
        if (p.advance) cx ^= 1;
        if (p.advance_y) cy ^= 1;
        PgmBpdnArgs<T> a;
        a.dk = this->dk;
        a.dtk = this->dtk;
        a.s = this->s;
        a.w = have_w ? w : nullptr;
        a.w_s = (T)p.w;
        a.wl1 = this->have_wl1 ? this->wl1 : nullptr;
        a.wl1_s = (T)p.wl1;
        a.x = xbuf(cx);
        a.xprv = xbuf(cx ^ 1);
        a.y = ybuf(cy);
        a.yprv = p.ymode == SPORCO_AMD_PGMB_Y_ROBUST ? ybuf(cy ^ 1) : nullptr;
        this->need(&g);
        a.g = g;
        if (p.ymode == SPORCO_AMD_PGMB_Y_ROBUST) {
            this->need(&zv);
            a.z = zv;
        }
        if (p.keep_zz) {
            this->need(&zz);
            a.zz = zz;
        }
        a.L = (T)p.L;
        a.lmbda = (T)p.lmbda;
        a.beta = (T)p.beta;
        a.tk = (T)p.tk;
        a.tt = (T)p.t;
        a.TT = (T)(p.tk + p.t);
        a.zc = (T)p.zc;
        a.phase = p.phase;
        a.ymode = p.ymode;
        a.nonneg = p.nonneg;
        a.revert = p.revert;
        a.z_update = p.z_update;
        a.cauchy = p.cauchy;
        a.bb = p.bb;
        a.form = this->form;
        a.M = this->M;
        a.N = this->N;
        a.K = this->K;
        a.KB = this->KB;
        a.partials = part_pgm;
        {
            ProfScope ps(this->prof, PS_BPDN_PGM_STEP);
            launch_bpdn_pgm_step<T>(this->st, a);
        }
        // (pgm_bpdn_sums order = the SPORCO_AMD_PGMB_* slots; the halves of f)
        // in two groups of the one reduction launch (a group holds eight sums)
        const int slots[8] = {0, 1, 2, 3, 4, 5, 6, 7}, slots_b[3] = {8, 9, 10};
        const double scales[8] = {0.5, 0.5, 1, 1, 1, 1, 1, 1}, ones[3] = {1, 1, 1};
        {
            ProfScope ps(this->prof, PS_FINALIZE);
            launch_finalize2(this->st, part_pgm, this->nb, kPgmBpdnSums, 8, slots, scales, part_pgm + 8, this->nb,
                             kPgmBpdnSums, 3, slots_b, ones, this->out_dev);
        }
        if (out_host) this->read_out(out_host);
    }

    void pgm_ystep(double beta, double gamma, int use_zz, int advance_y, double *out_host) override {
        if (use_zz) this->need(&zz);
        if (advance_y) cy ^= 1;
        int nby;
        {
            ProfScope ps(this->prof, PS_BPDN_PGM_YSTEP);
            nby = launch_bpdn_pgm_ystep<T>(this->st, xbuf(cx), xbuf(cx ^ 1), use_zz ? zz : nullptr, ybuf(cy), (T)beta,
                                           (T)gamma, (int64_t)this->M * this->K, part_y);
        }
        const int slots[1] = {SPORCO_AMD_PGMB_RS2};
        const double scales[1] = {1.0};
        finalize_read(part_y, nby, 1, 1, slots, scales, out_host);
    }
};

BpdnBase *make_pgm_bpdn(int dtype, int N, int M, int64_t K, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new PgmBpdn<float>(N, M, K, device, stream);
    if (dtype == SPORCO_AMD_F64) return new PgmBpdn<double>(N, M, K, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
