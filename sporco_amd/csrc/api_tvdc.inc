// api_tvdc.inc -- the handle of TVL2Deconv (sporco/admm/tvl2.py:377-702) and, in l1 mode, TVL1Deconv
// (sporco/admm/tvl1.py:403-758); kernels: csc_tvdc.h, transforms: rfft2 / irfft2 of fft.h on the generic
// chain.  Like api_tvd.inc it is included by csc_api.hip at namespace scope, below template Csc<T>; the stream, the
// sums, the profiler, the two transform plans and the ownership of every buffer are SideBase's (csc_impl.h).
// The arrays: S, Y, U (nb blocks), dY (l2) and the weights are (H, W, P); XH, RY, RU are (H, W, NZ, P) with
// NZ = 1 (l2) or 2 (l1); the spectra Sf, AHSf are (H, Wf, P), Af and |Af|^2 (H, Wf, PA) with PA = P (a kernel
// per plane) or 1 (one for all), the work spectrum (H, Wf, NZ, P).
template <typename T> struct Tvdc : TvdcBase {
    TvdPlan pl;
    const bool l1;
    const int nb, nz;               // blocks of Y and of U; planes of XH, RY, RU per image plane
    const int H, W, Wf;
    const int64_t P, PA;
    int64_t E, F;                   // H W P, H Wf P
    T *s = nullptr, *xh = nullptr, *y = nullptr, *u = nullptr, *dy = nullptr, *ry = nullptr, *ru = nullptr;
    T *wdf = nullptr, *wtv = nullptr, *aha = nullptr, *ch = nullptr, *cw = nullptr;
    cx<T> *wf = nullptr, *sf = nullptr, *ahsf = nullptr, *af = nullptr;
    bool have_wdf = false, have_wtv = false, have_s = false, have_a = false;
    int sblocks = 1;
    double *part_y = nullptr, *part_a = nullptr, *part_s = nullptr, *part_d = nullptr;

    Tvdc(int H_, int W_, int64_t P_, int C, bool vtv, bool l1_mode, int64_t PA_, int dev, void *stream)
        : TvdcBase(dev, stream), l1(l1_mode), nb(l1_mode ? 3 : 2), nz(l1_mode ? 2 : 1), H(H_), W(W_), Wf(W_ / 2 + 1),
          P(P_), PA(PA_) {
        SA_REQUIRE(PA == P || PA == 1, "tvdc: one kernel for all planes or one per plane");
        pl = tvd_plan(sizeof(T), H, W, P, C, vtv);
        E = pl.L * H;
        F = (int64_t)H * Wf * P;
        planH.init(H);
        planW.init(W);
        // (the refusal of a line that does not fit a workgroup's LDS comes here, not at the first iteration)
        fft_require_line_fits<T>(planW);
        fft_require_line_fits<T>(planH);
        s = dev_alloc<T>(E, true);
        for (T **p : {&xh, &ry, &ru}) *p = dev_alloc<T>(nz * E, true);
        for (T **p : {&y, &u}) *p = dev_alloc<T>(nb * E, true);
        if (!l1) dy = dev_alloc<T>(2 * E, true);
        aha = dev_alloc<T>((int64_t)H * Wf * PA, true);
        ch = dev_alloc<T>(H, true);
        cw = dev_alloc<T>(Wf, true);
        wf = dev_alloc<cx<T>>(nz * F, true);
        sf = dev_alloc<cx<T>>(F, true);
        ahsf = dev_alloc<cx<T>>(F, true);
        af = dev_alloc<cx<T>>((int64_t)H * Wf * PA, true);
        launch_tvdc_tables<T>(st, H, W, ch, cw);
        sblocks = tvdc_solve_blocks(solve_args(T(1)));
        part_y = dev_alloc<double>(kTvdSums * pl.blocks(), false);
        part_a = dev_alloc<double>(kTvdSums * pl.blocks(), false);
        part_s = dev_alloc<double>(kTvdcSolveSums * sblocks, false);
        part_d = dev_alloc<double>(sblocks, false);
        sync();
    }

    void plan(int64_t out[8]) override {
        out[0] = pl.cnt;
        out[1] = pl.items;
        out[2] = pl.strips;
        out[3] = pl.rows;
        out[4] = pl.nseg;
        // the columns a strip of 256 items covers (at least one)
        const int64_t per = pl.vtv ? pl.N : pl.P;
        out[5] = std::max<int64_t>(1, (int64_t)kTvdThreads * (pl.vtv ? 1 : pl.cnt) / per);
        // tvdc_solve: planes per access, workgroups
        out[6] = (sizeof(T) == 4 && P % 2 == 0) ? 2 : 1;
        out[7] = sblocks;
    }

    TvdcSolveArgs<T> solve_args(T rho) {
        TvdcSolveArgs<T> a;
        a.wf = wf;
        a.ahsf = ahsf;
        a.sf = sf;
        a.af = af;
        a.aha = aha;
        a.ch = ch;
        a.cw = cw;
        a.H = H;
        a.W = W;
        a.Wf = Wf;
        a.P = P;
        a.PA = PA;
        a.rho = rho;
        a.partials = part_s;
        return a;
    }

    T *var_buf(int var, int64_t *n) {
        *n = (var == SPORCO_AMD_TVDC_Y || var == SPORCO_AMD_TVDC_U) ? nb * E : E;
        switch (var) {
        case SPORCO_AMD_TVDC_S: return s;
        case SPORCO_AMD_TVDC_Y: return y;
        case SPORCO_AMD_TVDC_U: return u;
        case SPORCO_AMD_TVDC_WDF: return wdf;
        case SPORCO_AMD_TVDC_WTV: return wtv;
        default: throw Error(SPORCO_AMD_EINVAL, "tvdc: unknown array id");
        }
    }
    void upload(int var, const void *src, bool on_device) override {
        SA_REQUIRE(var != SPORCO_AMD_TVDC_X && var != SPORCO_AMD_TVDC_HX, "tvdc: X is the result of the x step, it is not set");
        if (var == SPORCO_AMD_TVDC_WDF || var == SPORCO_AMD_TVDC_WTV) {
            SA_REQUIRE(var == SPORCO_AMD_TVDC_WTV || l1, "tvdc: DFidWeight belongs to the l1 problem");
            bool &have = var == SPORCO_AMD_TVDC_WDF ? have_wdf : have_wtv;
            T *&w = var == SPORCO_AMD_TVDC_WDF ? wdf : wtv;
            have = src != nullptr;
            if (!have) return;
            SA_REQUIRE(var == SPORCO_AMD_TVDC_WDF || !pl.vtv, "tvdc: vector TV takes a scalar TVWeight");
            if (!w) w = dev_alloc<T>(E, false);
        }
        SA_REQUIRE(src != nullptr, "tvdc: null source");
        int64_t n;
        T *dst = var_buf(var, &n);
        SA_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (var == SPORCO_AMD_TVDC_S) {
            rfft2<T>(st, planW, planH, s, nullptr, T(0), sf, H, W, P);
            have_s = true;
            if (have_a) launch_tvdc_setup<T>(st, solve_args(T(1)), nullptr, ahsf);
            if (l1) {
                // || c ||^2 = || S ||^2 of the primal normaliser is constant: formed here, on the device, into a
                // slot of out_dev that no later finalize writes, so every read of the sums carries it
                launch_tvl1_s2<T>(st, s, pl, part_y);
                const int slot = SPORCO_AMD_OUT_C2;
                const double one = 1.0;
                launch_finalize(st, part_y, (int)pl.blocks(), 1, 1, &slot, &one, false, out_dev);
            }
        }
        sync();      // (the source may be pageable host memory, or a device array the caller frees next)
    }
    void download(int var, void *dst, bool on_device) override {
        SA_REQUIRE(dst != nullptr, "tvdc: null destination");
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (var == SPORCO_AMD_TVDC_X || var == SPORCO_AMD_TVDC_HX) {
            SA_REQUIRE(var == SPORCO_AMD_TVDC_X || l1, "tvdc: H X is kept by the l1 problem only");
            // plane group 0 (1) of the nz: H W runs of P elements, nz P apart
            const T *src = xh + (var == SPORCO_AMD_TVDC_HX ? P : 0);
            SA_HIP(hipMemcpy2DAsync(dst, sizeof(T) * P, src, sizeof(T) * P * nz, sizeof(T) * P, (size_t)H * W, kind, st));
        } else {
            int64_t n;
            const T *src = var_buf(var, &n);
            SA_REQUIRE(src != nullptr, "tvdc: this weight is a scalar");
            SA_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, kind, st));
        }
        sync();
    }
    // A of shape (ah, aw, PA), ah <= H, aw <= W, zero-padded to (H, W, PA) on the device and transformed
    void set_kernel(const void *src, int ah, int aw, bool on_device) override {
        SA_REQUIRE(src != nullptr && ah >= 1 && aw >= 1 && ah <= H && aw <= W, "tvdc: the kernel is no larger than the image");
        T *tmp = nullptr;
        const int64_t n = (int64_t)H * W * PA;
        SA_HIP(hipMalloc((void **)&tmp, sizeof(T) * n));
        try {
            SA_HIP(hipMemsetAsync(tmp, 0, sizeof(T) * n, st));
            SA_HIP(hipMemcpy2DAsync(tmp, sizeof(T) * W * PA, src, sizeof(T) * aw * PA, sizeof(T) * aw * PA, (size_t)ah,
                                    on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
            rfft2<T>(st, planW, planH, tmp, nullptr, T(0), af, H, W, PA);
            have_a = true;
            launch_tvdc_setup<T>(st, solve_args(T(1)), aha, have_s ? ahsf : nullptr);
            sync();
        } catch (...) {
            (void)hipStreamSynchronize(st);
            (void)hipFree(tmp);
            throw;
        }
        SA_HIP(hipFree(tmp));
    }

    TvdcArgs<T> args(const sporco_amd_tvdc_params &p) {
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        TvdcArgs<T> a;
        a.s = s;
        a.xh = xh;
        a.y = y;
        a.u = u;
        a.dy = (!l1 && p.want_rsdl) ? dy : nullptr;
        a.ry = ry;
        a.ru = ru;
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
    // the x step: Xf from the right-hand side RY - u_scale RU, then X (l1: X and H X)
    void xstep(const sporco_amd_tvdc_params &p) override {
        SA_REQUIRE(have_s && have_a, "tvdc: S and the kernel A are set before the first x step");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        {
            ProfScope ps(prof, PS_TVDC_RFFT2);
            rfft2<T>(st, planW, planH, ry, ru, (T)p.u_scale, wf, H, W, nz * P);
        }
        TvdcSolveArgs<T> a = solve_args((T)p.rho);
        a.want_dfid = (!l1 && p.want_stats) ? 1 : 0;
        a.want_lsc = p.lin_solve_check ? 1 : 0;
        {
            ProfScope ps(prof, PS_TVDC_SOLVE);
            launch_tvdc_solve<T>(st, a, l1);
        }
        {
            ProfScope ps(prof, PS_TVDC_IRFFT2);
            irfft2<T>(st, planW, planH, wf, wf, xh, H, W, nz * P);
        }
        if (a.want_dfid || a.want_lsc) {
            // (DFid with the Parseval scale 1 / (H W), rfl2norm2 of sporco/fft.py:449-484; not halved)
            const int slots[4] = {SPORCO_AMD_OUT_DFID, SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2,
                                  SPORCO_AMD_OUT_XRRS_B2};
            const double scales[4] = {1.0 / ((double)H * (double)W), 1, 1, 1};
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize(st, part_s, sblocks, kTvdcSolveSums, 4, slots, scales, false, out_dev);
        }
    }
    // relax + y step + u step, the adjoint arrays of the next right-hand side, and the dual residual's sums
    void ystep(const sporco_amd_tvdc_params &p, double *out_host) override {
        TvdcArgs<T> a = args(p);
        a.partials = part_y;
        {
            ProfScope ps(prof, PS_TVDC_YSTEP);
            launch_tvdc_ystep<T>(st, a, pl, l1);
        }
        a.partials = part_a;
        {
            ProfScope ps(prof, PS_TVDC_ADJOINT);
            launch_tvdc_adjoint<T>(st, a, pl, l1);
        }
        const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        if (l1) {
            const int slots_y[6] = {SPORCO_AMD_OUT_R2,  SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2,
                                    SPORCO_AMD_OUT_L21, SPORCO_AMD_OUT_U2,  SPORCO_AMD_OUT_DFID};
            const int slot_d = SPORCO_AMD_OUT_S2;
            const double scale_d = 1.0 / ((double)H * (double)W);
            if (p.want_rsdl) {
                // rho || A^T U || = rho || G^T U_g + H^T U_d || (tvl1.py:747-750), over spectra
                ProfScope ps(prof, PS_TVDC_DUAL);
                rfft2<T>(st, planW, planH, ru, nullptr, T(0), wf, H, W, 2 * P);
                TvdcSolveArgs<T> d = solve_args((T)p.rho);
                d.partials = part_d;
                launch_tvdc_dual<T>(st, d);
            }
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize2(st, part_y, (int)pl.blocks(), kTvdSums, 6, slots_y, ones, part_d, sblocks, 1,
                             p.want_rsdl ? 1 : 0, &slot_d, &scale_d, out_dev);
        } else {
            // (OUT_U2 = || G^T U ||^2: the normaliser of ADMM's own dual residual, admm.py:254-255)
            const int slots_y[4] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2, SPORCO_AMD_OUT_L21};
            const int slots_a[2] = {SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_U2};
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize2(st, part_y, (int)pl.blocks(), kTvdSums, 4, slots_y, ones, part_a, (int)pl.blocks(), kTvdSums,
                             2, slots_a, ones, out_dev);
        }
        read_out(out_host);
    }
    // RY, RU of the current Y, U (after an upload of either)
    void adjoint() override {
        sporco_amd_tvdc_params p = {1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1, 0, 0, 0};
        TvdcArgs<T> a = args(p);
        a.partials = part_a;
        ProfScope ps(prof, PS_TVDC_ADJOINT);
        launch_tvdc_adjoint<T>(st, a, pl, l1);
    }
};

TvdcBase *make_tvdc(int dtype, int H, int W, int64_t P, int C, bool vector_tv, bool l1, int64_t PA, int device,
                    void *stream) {
    if (dtype == SPORCO_AMD_F32) return new Tvdc<float>(H, W, P, C, vector_tv, l1, PA, device, stream);
    if (dtype == SPORCO_AMD_F64) return new Tvdc<double>(H, W, P, C, vector_tv, l1, PA, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
