// api_rtv.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvBPDNRecTV (sporco/admm/cbpdntv.py:733-1356), total variation of the
// reconstruction (csc_rtv.h).
    // While rtv_active, the handle's own VAR_Y / VAR_U hold the coefficient blocks (y0, u0) and
    // VAR_RTVY1 / VAR_RTVU1 the gradient blocks (y1, u1), (H, W, C, N, 2).  Beside them live the
    // spectra the x step and the residual norms read -- rfftn(y0), its predecessor and rfftn(u0), and
    // the same three of the adjoint maps Z = sum_i G_i^T v1_i -- kept current by rtv_dual.  All K-map
    // transforms are the generic chain's (fwd2 / inv2, natural layout) on every handle.
    bool rtv_active = false, rtv_uniform = true;
    T *rtv_w = nullptr;                        // Wtv, K values (0 on a padding filter)
    cx<T> *rtv_yf = nullptr, *rtv_yfp = nullptr, *rtv_uf = nullptr;      // (npix, CN, K)
    cx<T> *rtv_zyf = nullptr, *rtv_zyfp = nullptr, *rtv_zuf = nullptr;   // (npix, CN)
    cx<T> *rtv_rwf = nullptr;                  // sum_m w_m Df_m Xf_m, (npix, CN)
    T *rtv_rw = nullptr, *rtv_zy = nullptr, *rtv_zu = nullptr;           // (H, W, CN)
    double *rtv_part = nullptr;

    void rtv_release() {
        for (void *p : {(void *)rtv_yf, (void *)rtv_yfp, (void *)rtv_uf}) big_free(p);
        for (void *p : {(void *)rtv_w, (void *)rtv_zyf, (void *)rtv_zyfp, (void *)rtv_zuf, (void *)rtv_rwf,
                        (void *)rtv_rw, (void *)rtv_zy, (void *)rtv_zu, (void *)rtv_part})
            if (p) (void)hipFree(p);
        rtv_yf = rtv_yfp = rtv_uf = rtv_zyf = rtv_zyfp = rtv_zuf = rtv_rwf = nullptr;
        rtv_w = rtv_rw = rtv_zy = rtv_zu = nullptr;
        rtv_part = nullptr;
    }

    void rtv_setup(const double *tvw, int n) override {
        SA_REQUIRE(Cd == 1 && depth == 1 && !cplx, "RecTV: single-channel real dictionary, no volume handle");
        SA_REQUIRE(H >= 2 && W >= 2, "RecTV: images (both spatial extents >= 2)");
        SA_REQUIRE(tvw != nullptr && (n == 1 || n == Ku), "TVWeight: a scalar or one weight per filter");
        before_state_change();
        sync();
        std::vector<T> w((size_t)K, T(0));
        for (int k = 0; k < Ku; ++k) w[k] = (T)tvw[n == 1 ? 0 : k];
        rtv_uniform = true;
        for (int k = 1; k < Ku; ++k) rtv_uniform = rtv_uniform && w[k] == w[0];
        const size_t cs = sizeof(cx<T>) * (size_t)npix * CN, rs = sizeof(T) * (size_t)H * W * CN;
        if (!rtv_w) {
            SA_HIP(hipMalloc((void **)&rtv_w, sizeof(T) * K));
            for (cx<T> **p : {&rtv_zyf, &rtv_zyfp, &rtv_zuf, &rtv_rwf}) SA_HIP(hipMalloc((void **)p, cs));
            for (T **p : {&rtv_rw, &rtv_zy, &rtv_zu}) SA_HIP(hipMalloc((void **)p, rs));
            SA_HIP(hipMalloc((void **)&rtv_part, sizeof(double) * 8 * 2 * kMaxPartialBlocks));
            for (cx<T> **p : {&rtv_yf, &rtv_yfp, &rtv_uf}) big_alloc((void **)p, sizeof(cx<T>) * (size_t)EF);
        }
        SA_HIP(hipMemcpy(rtv_w, w.data(), sizeof(T) * K, hipMemcpyHostToDevice));
        for (cx<T> *p : {rtv_zyf, rtv_zyfp, rtv_zuf, rtv_rwf}) SA_HIP(hipMemsetAsync(p, 0, cs, st));
        for (cx<T> *p : {rtv_yf, rtv_yfp, rtv_uf}) SA_HIP(hipMemsetAsync(p, 0, sizeof(cx<T>) * (size_t)EF, st));
        SA_HIP(hipMemsetAsync(rtv_rw, 0, rs, st));
        (void)grad_term(0.0);     // (the separable GHG tables)
        // the two arrays each kernel writes at the same time: (y0, u0), and (y1, u1)
        place_var(SPORCO_AMD_VAR_U, {SPORCO_AMD_VAR_Y}, "U0");
        place_var(SPORCO_AMD_VAR_RTVY1, {}, "Y1");
        place_var(SPORCO_AMD_VAR_RTVU1, {SPORCO_AMD_VAR_RTVY1}, "U1");
        place_release_spares();
        rtv_active = true;
        // the spectra of whatever blocks the handle holds (zero on a fresh one)
        sporco_amd_admm_params p0{};
        rtv_dual(p0, out_dev_own);
        sync();
    }

    // (B^H diag(1, rho GHG) B + rho I) x = rho (Yf0 - Uf0) + B^H (Sf; rho (Zyf - Zuf)) (csc_rtv.h;
    // cbpdntv.py:1026-1094), X = irfftn(Xf) and rw = irfftn(sum_m w_m Df_m Xf_m)
    void rtv_xstep(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(rtv_active, "rtv_xstep without rtv_setup");
        SA_REQUIRE(p.rho > 0.0, "rtv_xstep: rho > 0");
        require_ready();
        before_state_change();
        x_written();
        xf_tiled = false;
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF);
        const GradTerm<T> gt = grad_term(0.0);
        RtvSolveArgs<T> a;
        a.yf = rtv_yf;
        a.uf = rtv_uf;
        a.xf = Xf;
        a.df = cv(SPORCO_AMD_VAR_DF);
        a.sf = cv(SPORCO_AMD_VAR_SF);
        a.zyf = rtv_zyf;
        a.zuf = rtv_zuf;
        a.rwf = rtv_rwf;
        a.gram = gram;
        a.tvw = rtv_w;
        a.ghh = gt.ghh;
        a.ghw = gt.ghw;
        a.rho = (T)p.rho;
        a.us = (T)p.u_scale;
        a.uniform = rtv_uniform ? 1 : 0;
        a.npix = npix;
        a.CN = CN;
        a.K = K;
        a.W = W;
        a.want_obj = ((p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y)) ? 1 : 0;
        a.want_xrrs = (p.flags & F_XRRS) ? 1 : 0;
        a.partials = part_a;
        int nb;
        {
            ProfScope ps(prof, PS_RTV_SOLVE);
            nb = launch_rtv_solve<T>(st, a);
        }
        if (a.want_obj || a.want_xrrs) finalize_solve(nb, 4, 1.0 / ((double)H * W), SPORCO_AMD_OUT_RGR, out_dev);
        inv2(Xf, work_buf(), rv(SPORCO_AMD_VAR_X), P);
        inv2(rtv_rwf, rtv_rwf, rtv_rw, CN);
    }

    void rtv_ystep(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(rtv_active, "rtv_ystep without rtv_setup");
        SA_REQUIRE(p.rho > 0.0, "rtv_ystep: rho > 0");
        before_read(SPORCO_AMD_VAR_X);
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        RtvYArgs<T> a;
        a.x = rv(SPORCO_AMD_VAR_X);
        a.y0 = rv(SPORCO_AMD_VAR_Y);
        a.u0 = rv(SPORCO_AMD_VAR_U);
        a.rw = rtv_rw;
        a.y1 = rv(SPORCO_AMD_VAR_RTVY1);
        a.u1 = rv(SPORCO_AMD_VAR_RTVU1);
        a.wl1 = wl1;
        a.rlx = (T)p.rlx;
        a.thr_l1 = (T)(p.lmbda / p.rho);
        a.thr_tv = (T)(p.mu / p.rho);
        a.us = (T)p.u_scale;
        a.geval_y = p.flags & F_GEVAL_Y;
        a.H = H;
        a.W = W;
        a.C = C;
        a.N = N;
        a.K = K;
        a.partials = rtv_part;
        int nb;
        {
            ProfScope ps(prof, PS_RTV_YSTEP);
            nb = launch_rtv_ystep<T>(st, a);
        }
        const int slots[5] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2, SPORCO_AMD_OUT_L1,
                              SPORCO_AMD_OUT_L21};
        const double scales[5] = {1, 1, 1, 1, 1};
        finalize(rtv_part, nb, 8, 5, slots, scales, out_dev);
    }

    // The spectra of the blocks as they stand -- rfftn(y0) (the previous one is kept), rfftn(u0) and
    // those of the adjoint maps of (y1, u1) -- and from them rho-free ||A^T (Y - Yprev)||^2 and
    // ||A^T U||^2 (admm.py:722-775); the data fidelity at y0 when fEvalX is off (cbpdntv.py:1110-1116).
    // Also the call that makes the handle consistent after the blocks were uploaded.
    void rtv_dual(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(rtv_active, "rtv_dual without rtv_setup");
        before_state_change();
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        std::swap(rtv_yf, rtv_yfp);
        std::swap(rtv_zyf, rtv_zyfp);
        {
            ProfScope ps(prof, PS_RTV_DUAL);
            launch_rtv_adjoint<T>(st, rv(SPORCO_AMD_VAR_RTVY1), rv(SPORCO_AMD_VAR_RTVU1), rtv_zy, rtv_zu, H, W, CN);
        }
        fwd2(rv(SPORCO_AMD_VAR_Y), nullptr, T(0), rtv_yf, P);
        fwd2(rv(SPORCO_AMD_VAR_U), nullptr, T(0), rtv_uf, P);
        fwd2(rtv_zy, nullptr, T(0), rtv_zyf, CN);
        fwd2(rtv_zu, nullptr, T(0), rtv_zuf, CN);
        RtvDualArgs<T> a;
        a.yf = rtv_yf;
        a.yfp = rtv_yfp;
        a.uf = rtv_uf;
        a.zyf = rtv_zyf;
        a.zyfp = rtv_zyfp;
        a.zuf = rtv_zuf;
        a.df = cv(SPORCO_AMD_VAR_DF);
        a.tvw = rtv_w;
        a.npix = npix;
        a.CN = CN;
        a.K = K;
        a.W = W;
        a.partials = part_a;
        int nb;
        {
            ProfScope ps(prof, PS_RTV_DUAL);
            nb = launch_rtv_dual<T>(st, a);
        }
        const int slots[2] = {SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_U2};
        const double scales[2] = {1.0 / ((double)H * W), 1.0 / ((double)H * W)};
        finalize(part_a, nb, 4, 2, slots, scales, out_dev);
        if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) {
            {
                ProfScope ps(prof, PS_OTHER);
                inner_df(rtv_yf);
                nb = launch_rfl2norm2<T>(st, innerb, cv(SPORCO_AMD_VAR_SF), npix, CNs, W, part_a);
            }
            const int fslots[1] = {SPORCO_AMD_OUT_DFID};
            const double fscales[1] = {1.0 / ((double)H * W)};
            finalize(part_a, nb, 1, 1, fslots, fscales, out_dev);
        }
    }
