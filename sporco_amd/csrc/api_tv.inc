// api_tv.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvBPDNScalarTV / ConvBPDNVectorTV (sporco/admm/cbpdntv.py): the three-block
// iterate of a handle and the two kernels around the x step (csc_tv.h).
    // While tv_active, VAR_TVY / VAR_TVU hold the blocks (y_0, y_1, y_L) of Y and U, and the handle's
    // own VAR_Y / VAR_U hold P = A^T Y and Q = A^T U: the staged x step (admm_xstep with
    // F_GRADREG, mu = rho, the grad-weight array Wtv^2) then transforms exactly the reference's
    // right-hand side rho (YUf_L + Wtv sum_i conj(Gf_i) YUf_i) (cbpdntv.py:281-296).
    bool tv_active = false, tv_vector = false;
    bool tv_uniform = true;     // every filter has the same TVWeight: the x step is ConvBPDNGradReg's
    T *tv_w = nullptr;          // Wtv, K values
    double *tv_part = nullptr, *tv_gn = nullptr;
    int64_t tv_part_cap = 0;
    TvPlan tv_pl;

    void tv_release() {
        if (tv_w) (void)hipFree(tv_w);
        if (tv_part) (void)hipFree(tv_part);
        if (tv_gn) (void)hipFree(tv_gn);
        tv_gn = nullptr;
        tv_w = nullptr;
        tv_part = nullptr;
    }

    void tv_setup(const double *tvw, int n, bool vector_tv) override {
        SA_REQUIRE(Cd == 1 && depth == 1 && !cplx, "TV regularisation: single-channel real dictionary, no volume handle");
        SA_REQUIRE(tvw != nullptr && (n == 1 || n == Ku), "TVWeight: a scalar or one weight per filter");
        before_state_change();
        sync();
        tv_pl = tv_plan<T>(H, W, CN, K);
        // (a padding filter gets weight 0: its gradient blocks stay exactly zero)
        std::vector<T> w((size_t)K, T(0)), w2((size_t)Ku);
        for (int k = 0; k < Ku; ++k) {
            const double v = tvw[n == 1 ? 0 : k];
            w[k] = (T)v;
            w2[k] = (T)(v * v);
        }
        tv_uniform = true;
        for (int k = 1; k < Ku; ++k) tv_uniform = tv_uniform && w[k] == w[0];
        if (!tv_w) SA_HIP(hipMalloc((void **)&tv_w, sizeof(T) * K));
        if (!tv_gn) SA_HIP(hipMalloc((void **)&tv_gn, sizeof(double) * kOutSlots));
        SA_HIP(hipMemcpy(tv_w, w.data(), sizeof(T) * K, hipMemcpyHostToDevice));
        set_grad_weight(w2.data());      // the x step's diagonal is rho Wtv^2 GHGf + rho (cbpdntv.py:291)
        if (tv_pl.blocks > tv_part_cap) {
            if (tv_part) SA_HIP(hipFree(tv_part));
            tv_part = nullptr;
            SA_HIP(hipMalloc((void **)&tv_part, sizeof(double) * 8 * tv_pl.blocks));
            tv_part_cap = tv_pl.blocks;
        }
        // the two arrays each kernel writes at the same time: (Y, U) blocks, and (P, Q)
        place_var(SPORCO_AMD_VAR_TVY, {}, "TVY");
        place_var(SPORCO_AMD_VAR_TVU, {SPORCO_AMD_VAR_TVY}, "TVU");
        place_var(SPORCO_AMD_VAR_U, {SPORCO_AMD_VAR_Y}, "Q");
        place_release_spares();
        sync();
        tv_vector = vector_tv;
        tv_active = true;
    }

    // (D^H D + rho Wtv^2 GHGf + rho) x = D^H s + rho A^T (Y - U) on VAR_Y = A^T Y, VAR_U = A^T U
    // (cbpdntv.py:277-310): the staged gradient-regularised x step; with different weights per
    // filter the reference's own arithmetic instead (csc_tv.h launch_tv_sm_ref), on the generic chain
    void tv_xstep(const sporco_amd_admm_params &pin, double *out_dev) override {
        SA_REQUIRE(tv_active, "tv_xstep without tv_setup");
        sporco_amd_admm_params p = pin;
        p.mu = p.rho;
        p.flags |= F_GRADREG | F_KEEP_X;
        before_state_change();
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        if (tv_uniform) {
            xstep_impl(p, out_dev);
            return;
        }
        require_ready();
        x_written();
        t_ready = false;
        xf_tiled = false;
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF);
        fwd2(rv(SPORCO_AMD_VAR_Y), rv(SPORCO_AMD_VAR_U), (T)p.u_scale, Xf, P);
        TvSmArgs<T> a;
        a.xf = Xf;
        a.df = cv(SPORCO_AMD_VAR_DF);
        a.sf = cv(SPORCO_AMD_VAR_SF);
        a.g = grad_term(p.mu);
        a.rho = (T)p.rho;
        a.npix = npix;
        a.CN = CN;
        a.K = K;
        a.W = W;
        a.want_obj = (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y);
        a.want_xrrs = (p.flags & F_XRRS) ? 1 : 0;
        a.partials = part_a;
        int nb;
        {
            ProfScope ps(prof, PS_SM_SOLVE);
            nb = launch_tv_sm_ref<T>(st, a);
        }
        if (a.want_obj || a.want_xrrs) finalize_solve(nb, 4, 1.0 / ((double)H * W), SPORCO_AMD_OUT_RGR, out_dev);
        inv2(Xf, work_buf(), rv(SPORCO_AMD_VAR_X), P);
    }

    TvArgs<T> tv_args() {
        TvArgs<T> a;
        a.y = rv(SPORCO_AMD_VAR_TVY);
        a.u = rv(SPORCO_AMD_VAR_TVU);
        a.tvw = tv_w;
        a.vector_tv = tv_vector;
        a.H = H;
        a.W = W;
        a.C = C;
        a.N = N;
        a.K = K;
        a.partials = tv_part;
        return a;
    }

    void tv_ystep(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(tv_active, "tv_ystep without tv_setup");
        SA_REQUIRE(p.rho > 0.0, "tv_ystep: rho > 0");
        before_read(SPORCO_AMD_VAR_X);
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        TvArgs<T> a = tv_args();
        a.x = rv(SPORCO_AMD_VAR_X);
        a.wl1 = wl1;
        a.rlx = (T)p.rlx;
        a.thr_l1 = (T)(p.lmbda / p.rho);
        a.thr_tv = (T)(p.mu / p.rho);
        a.u_scale = (T)p.u_scale;
        a.geval_y = p.flags & F_GEVAL_Y;
        int64_t nb;
        {
            ProfScope ps(prof, PS_TV_YSTEP);
            if (!tv_vector) {
                // scalar TV: ||(AX + U)_{0,1}||^2 over the whole array first (csc_tv.h)
                a.norm_pass = true;
                nb = launch_tv_ystep<T>(st, a, tv_pl);
                SA_HIP(hipMemsetAsync(tv_gn, 0, sizeof(double) * kOutSlots, st));
                const int s0[1] = {0};
                const double c0[1] = {1};
                launch_finalize(st, tv_part, (int)nb, 8, 1, s0, c0, false, tv_gn);
                a.norm_pass = false;
                a.gn2 = tv_gn;
            }
            nb = launch_tv_ystep<T>(st, a, tv_pl);
        }
        const int slots[5] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2, SPORCO_AMD_OUT_L1,
                              SPORCO_AMD_OUT_L21};
        const double scales[5] = {1, 1, 1, 1, 1};
        finalize(tv_part, (int)nb, 8, 5, slots, scales, out_dev);
        // data fidelity at y_L (fEvalX False, cbpdntv.py:325-331)
        if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) dfid_at(a.y + 2 * E, out_dev);
    }

    void tv_adjoint(double u_scale, double *out_dev) override {
        SA_REQUIRE(tv_active, "tv_adjoint without tv_setup");
        before_state_change();
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        TvArgs<T> a = tv_args();
        a.p = rv(SPORCO_AMD_VAR_Y);
        a.q = rv(SPORCO_AMD_VAR_U);
        a.u_scale = (T)u_scale;
        int64_t nb;
        {
            ProfScope ps(prof, PS_TV_ADJOINT);
            nb = launch_tv_adjoint<T>(st, a, tv_pl);
        }
        const int slots[2] = {SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_U2};
        const double scales[2] = {1, 1};
        finalize(tv_part, (int)nb, 8, 2, slots, scales, out_dev);
    }
