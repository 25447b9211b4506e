// api_tvd.inc -- the handle of TVL2Denoise (sporco/admm/tvl2.py:27-372; kernels: csc_tvd.h).  Unlike the
// other api_*.inc files this one is included by csc_api.hip at namespace scope, BELOW template Csc<T>:
// the class has no dictionary and no transform and does not share a CSC solver's state.
// l1 mode (sporco_amd_tvl1_create): TVL1Denoise (sporco/admm/tvl1.py:27-399) -- three blocks in Y and U, no
// dY, the y step and the adjoint are the tvl1_* kernels, the sweeps run with rho = 1 and a unit DFidWeight.
template <typename T> struct Tvd : TvdBase {
    TvdPlan pl;
    const bool l1;
    const int nb;                   // blocks of Y and of U: 2, or 3 in l1 mode
    int64_t E;                      // H W P
    T *s = nullptr, *x[2] = {nullptr, nullptr}, *y = nullptr, *u = nullptr, *dy = nullptr, *pd = nullptr, *q = nullptr;
    T *wdf = nullptr, *wtv = nullptr;
    bool have_wdf = false, have_wtv = false;
    int cur = 0;                    // x[cur] is X
    double *part_a = nullptr, *part_b = nullptr;

    Tvd(int H, int W, int64_t P, int C, bool vtv, bool l1_mode, int dev, void *stream)
        : TvdBase(dev, stream), l1(l1_mode), nb(l1_mode ? 3 : 2) {
        pl = tvd_plan(sizeof(T), H, W, P, C, vtv);
        E = pl.L * H;
        for (T **p : {&s, &x[0], &x[1], &pd, &q}) *p = dev_alloc<T>(E, true);
        for (T **p : {&y, &u}) *p = dev_alloc<T>(nb * E, true);
        if (!l1) dy = dev_alloc<T>(2 * E, true);
        part_a = dev_alloc<double>(kTvdSums * pl.blocks(), false);
        part_b = dev_alloc<double>(kTvdSums * pl.blocks(), false);
    }

    void plan(int64_t out[6]) override {
        out[0] = pl.cnt;
        out[1] = pl.items;
        out[2] = pl.strips;
        out[3] = pl.rows;
        out[4] = pl.nseg;
        // the columns a strip of 256 items covers (at least one)
        const int64_t per = pl.vtv ? pl.N : pl.P;
        out[5] = std::max<int64_t>(1, (int64_t)kTvdThreads * (pl.vtv ? 1 : pl.cnt) / per);
    }

    T *var_buf(int var, int64_t *n) {
        *n = (var == SPORCO_AMD_TVD_Y || var == SPORCO_AMD_TVD_U) ? nb * E : E;
        switch (var) {
        case SPORCO_AMD_TVD_S: return s;
        case SPORCO_AMD_TVD_X: return x[cur];
        case SPORCO_AMD_TVD_Y: return y;
        case SPORCO_AMD_TVD_U: return u;
        case SPORCO_AMD_TVD_WDF: return wdf;
        case SPORCO_AMD_TVD_WTV: return wtv;
        default: throw Error(SPORCO_AMD_EINVAL, "tvd: unknown array id");
        }
    }
    void upload(int var, const void *src, bool on_device) override {
        if (var == SPORCO_AMD_TVD_WDF || var == SPORCO_AMD_TVD_WTV) {
            bool &have = var == SPORCO_AMD_TVD_WDF ? have_wdf : have_wtv;
            T *&w = var == SPORCO_AMD_TVD_WDF ? wdf : wtv;
            have = src != nullptr;
            if (!have) return;
            SA_REQUIRE(var == SPORCO_AMD_TVD_WDF || !pl.vtv, "tvd: vector TV takes a scalar TVWeight");
            if (!w) w = dev_alloc<T>(E, false);
        }
        SA_REQUIRE(src != nullptr, "tvd: null source");
        int64_t n;
        T *dst = var_buf(var, &n);
        SA_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (var == SPORCO_AMD_TVD_S) {
            SA_HIP(hipMemcpyAsync(x[cur], s, sizeof(T) * n, hipMemcpyDeviceToDevice, st));
            if (l1) {
                // || c ||^2 = || S ||^2 of the primal normaliser is constant: formed here, on the device, into a
                // slot of out_dev that no later finalize writes, so every read of the sums carries it
                launch_tvl1_s2<T>(st, s, pl, part_a);
                const int slot = SPORCO_AMD_OUT_C2;
                const double one = 1.0;
                launch_finalize(st, part_a, (int)pl.blocks(), 1, 1, &slot, &one, false, out_dev);
            }
        }
        sync();      // (the source may be pageable host memory, or a device array the caller frees next)
    }
    void download(int var, void *dst, bool on_device) override {
        SA_REQUIRE(dst != nullptr, "tvd: null destination");
        int64_t n;
        const T *src = var_buf(var, &n);
        SA_REQUIRE(src != nullptr, "tvd: this weight is a scalar");
        SA_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        sync();
    }

    TvdArgs<T> args(const sporco_amd_tvd_params &p) {
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        TvdArgs<T> a;
        a.s = s;
        a.xin = x[cur];
        a.xout = x[cur ^ 1];
        a.y = y;
        a.u = u;
        a.dy = dy;
        a.pd = pd;
        a.q = q;
        a.wdf = have_wdf ? wdf : nullptr;
        a.wtv = have_wtv ? wtv : nullptr;
        a.wdf_s = (T)p.wdf;
        a.wtv_s = (T)p.wtv;
        a.rho = (T)p.rho;
        a.thr = (T)((T)p.lmbda / (T)p.rho);
        a.rlx = (T)p.rlx;
        a.u_scale = (T)p.u_scale;
        a.geval_y = p.geval_y;
        return a;
    }
    void sweeps(const sporco_amd_tvd_params &p, int n) override {
        for (int i = 0; i < n; ++i) {
            ProfScope ps(prof, PS_TVD_SWEEP);
            TvdArgs<T> a = args(p);
            if (l1) {      // (tvl1.py:252-253: GaussSeidelStep with rho = 1 and W2 = 1)
                a.rho = T(1);
                a.wdf = nullptr;
                a.wdf_s = T(1);
            }
            launch_tvd_sweep<T>(st, a, pl);
            cur ^= 1;
        }
    }
    void gsres(const sporco_amd_tvd_params &p, double *out_host) override {
        TvdArgs<T> a = args(p);
        a.partials = part_a;
        {
            ProfScope ps(prof, l1 ? PS_TVL1_YSTEP : PS_TVD_YSTEP);
            if (l1) launch_tvl1_ystep<T>(st, a, pl, true);
            else launch_tvd_ystep<T>(st, a, pl, true);
        }
        const int slots[3] = {SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2, SPORCO_AMD_OUT_XRRS_B2};
        const double scales[3] = {1, 1, 1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize(st, part_a + 5, (int)pl.blocks(), kTvdSums, 3, slots, scales, false, out_dev);
        }
        read_out(out_host);
    }
    void ystep(const sporco_amd_tvd_params &p, double *out_host) override {
        TvdArgs<T> a = args(p);
        a.partials = part_a;
        {
            ProfScope ps(prof, l1 ? PS_TVL1_YSTEP : PS_TVD_YSTEP);
            if (l1) launch_tvl1_ystep<T>(st, a, pl, false);
            else launch_tvd_ystep<T>(st, a, pl, false);
        }
        a.partials = part_b;
        {
            ProfScope ps(prof, l1 ? PS_TVL1_ADJOINT : PS_TVD_ADJOINT);
            if (l1) launch_tvl1_adjoint<T>(st, a, pl);
            else launch_tvd_adjoint<T>(st, a, pl);
        }
        const int slots_a[8] = {SPORCO_AMD_OUT_R2,  SPORCO_AMD_OUT_AX2,     SPORCO_AMD_OUT_Y2,       SPORCO_AMD_OUT_DFID,
                                SPORCO_AMD_OUT_L21, SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2, SPORCO_AMD_OUT_XRRS_B2};
        const int slots_b[2] = {SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_U2};
        const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize2(st, part_a, (int)pl.blocks(), kTvdSums, 8, slots_a, ones, part_b, (int)pl.blocks(), kTvdSums,
                             2, slots_b, ones, out_dev);
        }
        read_out(out_host);
    }
    void adjoint() override {
        sporco_amd_tvd_params p = {1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1};
        TvdArgs<T> a = args(p);
        a.partials = part_b;
        // (dY is whatever the last y step left, or zero: its sum is not read)
        ProfScope ps(prof, l1 ? PS_TVL1_ADJOINT : PS_TVD_ADJOINT);
        if (l1) launch_tvl1_adjoint<T>(st, a, pl);
        else launch_tvd_adjoint<T>(st, a, pl);
    }
};

TvdBase *make_tvd(int dtype, int H, int W, int64_t P, int C, bool vector_tv, bool l1, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new Tvd<float>(H, W, P, C, vector_tv, l1, device, stream);
    if (dtype == SPORCO_AMD_F64) return new Tvd<double>(H, W, P, C, vector_tv, l1, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
