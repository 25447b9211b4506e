// api_l1l1.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvL1L1Grd (sporco/admm/cbpdn.py:2488-2774), l1 data fidelity with l1 and gradient
// regularisation on the two-block state of ConvBPDNMaskDcpl (csc_l1l1.h).
    // The state is api_maskdcpl.inc's (mdcpl_init; block 1 in VAR_Y / VAR_U, block 0 in VAR_MY0 /
    // VAR_MU0), the mask, L1Weight and GradWeight the handle's own.  Generic transforms on every
    // shape.  Beside the state: Yprev - Y of the two blocks (block 1 in the relaxation buffer VAR_AX,
    // dead inside this iteration) and the spectrum of u0, for the dual residual.
    T *l1_dy0 = nullptr;            // y0prev - y0                           (H, W, Cs N)
    cx<T> *l1_u0f = nullptr;        // rfftn(u0)                             (npix, Cs N)

    void l1l1_release() {
        if (l1_dy0) (void)hipFree(l1_dy0);
        if (l1_u0f) (void)hipFree(l1_u0f);
        l1_dy0 = nullptr;
        l1_u0f = nullptr;
    }

    void l1l1_iter(const sporco_amd_admm_params &p, double *out_dev) override {
        require_ready();
        SA_REQUIRE(md_s != nullptr, "mdcpl_init must be called first");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        SA_REQUIRE(p.mu >= 0.0, "mu must not be negative");
        SA_REQUIRE(!(p.flags & (F_JOINT | F_AMS)), "flag not valid for ConvL1L1Grd");
        SA_REQUIRE(depth == 1 && !cplx, "ConvL1L1Grd: real data, no volume handle");
        SA_REQUIRE(Cd <= kL1MaxCd, "ConvL1L1Grd: at most 8 dictionary channels");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        before_state_change();
        x_written();
        xf_tiled = false;
        const int64_t ns = (int64_t)H * W * CNs;
        const T us = (T)p.u_scale;
        const bool want_dual = p.flags & F_RESID;
        T *Y1 = rv(SPORCO_AMD_VAR_Y), *U1 = rv(SPORCO_AMD_VAR_U), *X = rv(SPORCO_AMD_VAR_X);
        T *Y0 = rv(SPORCO_AMD_VAR_MY0), *U0 = rv(SPORCO_AMD_VAR_MU0);
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF), *Df = cv(SPORCO_AMD_VAR_DF);
        cx<T> *Vf = cv(SPORCO_AMD_VAR_VF);
        if (want_dual && !l1_dy0) {
            SA_HIP(hipMalloc((void **)&l1_dy0, sizeof(T) * ns));
            SA_HIP(hipMalloc((void **)&l1_u0f, sizeof(cx<T>) * npix * CNs));
        }
        // x step: b = conj(Df) rfftn(y0 - u0 + s) + rfftn(y1 - u1);
        // (D^H D + (mu / rho) Wgrd GHG + I) Xf = b   (cbpdn.py:2676-2699)
        {
            ProfScope ps(prof, PS_OTHER);
            launch_md_pre<T>(st, Y0, U0, md_s, sreal, us, ns);
        }
        fwd2(sreal, nullptr, T(0), innerb, CNs);
        fwd2(Y1, U1, us, Vf, P);
        const bool obj = p.flags & F_OBJ, xr = p.flags & F_XRRS;
        const double mu_eff = p.mu / p.rho;
        const GradTerm<T> gt = grad_term(mu_eff);
        // (the tables of the multi-channel solve hold the diagonal: a change of rho moves mu / rho and
        // rebuilds them; partial 0 is the solve's own residual against the block-0 spectrum: not a
        // statistic here)
        int nb = generic_solve(Vf, Xf, innerb, T(1), obj, xr, &gt, mu_eff);
        if (obj || xr) finalize_solve(nb, 5, 0.0, SPORCO_AMD_OUT_RGRX, out_dev);
        inv2(Xf, work_buf(), X, P);
        // block 0: AXnr = D x
        {
            ProfScope ps(prof, PS_OTHER);
            inner_df(Xf);
        }
        inv2(innerb, innerb, sreal, CNs);
        // block 1: relax, y1 = prox_l1 (+ NonNegCoef / NoBndryCross), u1, the sums, Yprev - Y
        T *dy1 = want_dual ? rv(SPORCO_AMD_VAR_AX) : nullptr;
        PostParams<T> pp = post_params(p, X, Y1, U1);
        pp.dy_out = dy1;
        {
            ProfScope ps(prof, PS_ADMM_POST);
            nb = launch_admm_post<T>(st, pp, part_b);
        }
        finalize_post(part_b, nb, 6, false, out_dev);
        L1Y0Args<T> ya;
        ya.ax0nr = sreal;
        ya.y0 = Y0;
        ya.u0 = U0;
        ya.s = md_s;
        ya.dy0 = want_dual ? l1_dy0 : nullptr;
        ya.w = have_wdat ? wdat : Weight<T>();
        ya.rho = (T)p.rho;
        ya.rlx = (T)p.rlx;
        ya.us = us;
        ya.geval_y = (p.flags & F_GEVAL_Y) ? 1 : 0;
        ya.H = H;
        ya.W = W;
        ya.C = Cs;
        ya.N = N;
        {
            ProfScope ps(prof, PS_L1L1_Y0STEP);
            nb = launch_l1l1_y0step<T>(st, ya, part_a);
        }
        {
            const int slots[5] = {SPORCO_AMD_OUT_L21, SPORCO_AMD_OUT_RGR, SPORCO_AMD_OUT_CNSTR,
                                  SPORCO_AMD_OUT_CGIT, SPORCO_AMD_OUT_DFID};
            const double scales[5] = {1, 1, 1, 1, 1};
            finalize(part_a, nb, 5, 5, slots, scales, out_dev);
        }
        if (want_dual) {
            // s = rho ||A^T (Yprev - Y)||, sn = rho ||A^T U|| (cbpdn.py:2753-2763): four forward
            // transforms, then both half-spectrum Parseval sums in one read-only pass
            cx<T> *Gf = cv(SPORCO_AMD_VAR_GF);
            fwd2(l1_dy0, nullptr, T(0), innerb, CNs);
            fwd2(U0, nullptr, T(0), l1_u0f, CNs);
            fwd2(dy1, nullptr, T(0), Vf, P);
            fwd2(U1, nullptr, T(0), Gf, P);
            L1DualArgs<T> da;
            da.df = Df;
            da.dy0f = innerb;
            da.u0f = l1_u0f;
            da.dy1f = Vf;
            da.u1f = Gf;
            da.npix = npix;
            da.Cd = Cd;
            da.CN = CN;
            da.K = K;
            da.W = W;
            da.partials = part_b;
            {
                ProfScope ps(prof, PS_L1L1_DUAL);
                nb = launch_l1l1_dual<T>(st, da);
            }
            const int slots[2] = {SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_SN2};
            const double scales[2] = {1.0 / ((double)H * W), 1.0 / ((double)H * W)};
            finalize(part_b, nb, 2, 2, slots, scales, out_dev);
        }
    }
