// api_maskdcpl.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ADMM sparse coding with mask decoupling (ConvBPDNMaskDcpl).
    // ---- ADMM with mask decoupling (ConvBPDNMaskDcpl) ---------------------------------------
    void mdcpl_init(const void *S) override {
        SA_REQUIRE(S != nullptr, "S is null");
        const size_t nb = sizeof(T) * (int64_t)H * W * CNs;
        if (!md_s) SA_HIP(hipMalloc((void **)&md_s, nb));
        SA_HIP(hipMemcpyAsync(md_s, S, nb, hipMemcpyHostToDevice, st));
        before_state_change();
        SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_Y), 0, sizeof(T) * E, st));
        SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_U), 0, sizeof(T) * E, st));
        SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_MY0), 0, nb, st));
        SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_MU0), 0, nb, st));
        sync();
    }

    // The iteration on the register-resident kernels of the unmasked class (round 4): float32,
    // H and W in {128, 256, 512} or (round 6) a mixed-radix length, even K <= 64, single-channel dictionary.
    //   block 0 -> signal spectrum:  md_pre, a signal-sized 2-D FFT, re-laid tile-major
    //   rows_fwd                     T = rfft_W(y1 - s u1)
    //   fused_cols                   column FFT, Sherman-Morrison with rho = 1 and that spectrum in
    //                                Sf's place, column IFFT; its multipliers (one per frequency and
    //                                image: signal sized) are kept, D x = Sf' - coef
    //   rows_inv_post                irfft_W, relax, prox_l1 (+ options), dual update of block 1, sums
    //   block 0                      D x to the spatial domain (signal sized), md_y0step
    //   dual residual (F_RESID)      rho ||A^T u|| needs the 2-D spectrum of the NEW u1: the epilogue
    //                                emits its row spectra into the scratch spectrum (emit_u), and a
    //                                column kernel transforms them and sums |conj(Df) rfftn(u0) +
    //                                rfftn(u1)|^2 in registers (one read pass, nothing written)
    // against the generic chain's four 2-D FFTs of X-sized arrays plus their glue passes.
    cx<T> *md_sft = nullptr, *md_coef = nullptr;
    // Block 0 given AXnr = D x in sreal: relax, y0, u0 and the five sums of the block.  y0 is the
    // mask-decoupling division (md_y0step) or -- ball, ConvMinL1InL2Ball -- the projection of
    // AX0 + U0 - S onto the l2 ball of radius p.mu, one ball per channel and image with the norm
    // over the image plane (csc_ball.h: two passes and the totals between them).  The ball class
    // has no data mask and leaves OUT_DFID to the constraint measure.
    double *ball_ws = nullptr;
    int64_t ball_ws_n = 0;
    void md_block0(const sporco_amd_admm_params &p, double *out_dev, bool ball) {
        T *Y0 = rv(SPORCO_AMD_VAR_MY0), *U0 = rv(SPORCO_AMD_VAR_MU0);
        const T us = (T)p.u_scale;
        int nb;
        if (ball) {
            const BallGeom g = ball_geom(sizeof(T), 1, (int64_t)H * W, CNs);
            if (ball_ws_n < g.workspace_doubles()) {
                if (ball_ws) SA_HIP(hipFree(ball_ws));
                ball_ws = nullptr;
                ball_ws_n = 0;
                SA_HIP(hipMalloc((void **)&ball_ws, sizeof(double) * g.workspace_doubles()));
                ball_ws_n = g.workspace_doubles();
            }
            BallArgs<T> ba;
            ba.ax0nr = sreal;
            ba.y0 = Y0;
            ba.u0 = U0;
            ba.s = md_s;
            ba.eps = p.mu;
            ba.rlx = (T)p.rlx;
            ba.us = us;
            ba.geval_y = (p.flags & F_GEVAL_Y) ? 1 : 0;
            ba.ws = ball_ws;
            {
                ProfScope ps(prof, PS_BALL_NORMS);
                launch_ball_norms<T>(st, ba, g);
                launch_ball_totals(st, ball_ws, g);
            }
            {
                ProfScope ps(prof, PS_BALL_Y0STEP);
                nb = launch_ball_y0step<T>(st, ba, g, part_a);
            }
        } else {
            MdY0Args<T> ya;
            ya.ax0nr = sreal;
            ya.y0 = Y0;
            ya.u0 = U0;
            ya.s = md_s;
            ya.w = have_wdat ? wdat : Weight<T>();
            ya.rho = (T)p.rho;
            ya.rlx = (T)p.rlx;
            ya.us = us;
            ya.geval_y = (p.flags & F_GEVAL_Y) ? 1 : 0;
            ya.H = H;
            ya.W = W;
            ya.C = Cs;
            ya.N = N;
            ProfScope ps(prof, PS_OTHER);
            nb = launch_md_y0step<T>(st, ya, part_a);
        }
        const int slots[5] = {SPORCO_AMD_OUT_L21, SPORCO_AMD_OUT_RGR, SPORCO_AMD_OUT_CNSTR,
                              SPORCO_AMD_OUT_CGIT, SPORCO_AMD_OUT_DFID};
        const double scales[5] = {1, 1, 1, 1, 1};
        finalize(part_a, nb, 5, 5, slots, scales, out_dev);
    }

    bool mdcpl_fused_ok(const sporco_amd_admm_params &p) const {
        return std::is_same<T, float>::value && rows_ok && mr_ok(p) && fused && !tail_mode && !fused_mc && Cd == 1 &&
               !(p.flags & F_XRRS) && p.lmbda >= 0.0 && !sw.md_generic;
    }
    void mdcpl_iter_fused(const sporco_amd_admm_params &p, double *out_dev, bool ball) {
        const int64_t ns = (int64_t)H * W * CNs, nsf = npix * CN;
        const T us = (T)p.u_scale;
        T *Y1 = rv(SPORCO_AMD_VAR_Y), *U1 = rv(SPORCO_AMD_VAR_U), *X = rv(SPORCO_AMD_VAR_X);
        T *Y0 = rv(SPORCO_AMD_VAR_MY0), *U0 = rv(SPORCO_AMD_VAR_MU0);
        if (!md_sft) {
            SA_HIP(hipMalloc((void **)&md_sft, sizeof(cx<T>) * nsf));
            SA_HIP(hipMalloc((void **)&md_coef, sizeof(cx<T>) * nsf));
        }
        {
            ProfScope ps(prof, PS_OTHER);
            launch_md_pre<T>(st, Y0, U0, md_s, sreal, us, ns);
        }
        fwd2(sreal, nullptr, T(0), innerb, CNs);
        {
            ProfScope ps(prof, PS_OTHER);
            launch_permute_ab<cx<T>>(st, innerb, md_sft, H, (int64_t)Wf * CN, 1);
        }
        launch_rows_fwd_on(Y1, U1, us);
        t_ready = false;
        // (the system with rho = 1 and the spectrum of block 0 in Sf's place; its multipliers kept)
        auto fa = fused_cols_args(1.0);
        fa.sft = md_sft;
        fa.coef_out = md_coef;
        {
            ProfScope ps(prof, PS_FUSED_COLS);
            part_f_rows = (int)launch_fused_cols<T>(st, fa);
        }
        xf_tiled = true;
        // D x = Sf' - rho coef (the kernel's Df.xf - Sf = -rho coef, rho = 1), back to (H, Wf, CN)
        {
            ProfScope ps(prof, PS_OTHER);
            launch_lincomb<T>(st, md_coef, T(1), md_sft, T(-1), md_coef, T(0), nullptr, nsf);
            launch_permute_ab<cx<T>>(st, md_coef, innerb, (int64_t)Wf * CN, H, 1);
        }
        inv2(innerb, innerb, sreal, CNs);
        // block 1 through the row epilogue, in place ((Y, U) form), X kept for its readers
        // with residuals wanted, the epilogue also leaves the row spectra of the NEW u1 in the
        // scratch spectrum (it has them in registers): the dual residual's input, for one write
        // pass instead of a row pass of its own over u1
        const bool want_dual = p.flags & F_RESID;
        cx<T> *wk = want_dual ? work_buf() : nullptr;
        auto pa = rows_post_args(p);
        pa.t_next = wk;
        pa.emit_u = want_dual ? 1 : 0;
        pa.y = Y1;
        pa.u = U1;
        pa.y_out = Y1;
        pa.u_out = U1;
        pa.x = (p.flags & F_KEEP_X) ? X : nullptr;
        pa.thr = (T)(p.lmbda / p.rho);
        pa.u_scale = us;
        int64_t nt;
        {
            ProfScope ps(prof, PS_ROWS_INV_POST);
            nt = launch_rows_inv_post<T>(st, pa);
        }
        // X is written on request only (F_KEEP_X); otherwise it is one row pass away for as long
        // as the Xf buffer keeps this iteration's intermediate (materialize_x)
        x_written();
        md_x_pending = !(p.flags & F_KEEP_X);
        int nb;
        finalize_post(part_rows, (int)nt, 6, false, out_dev);
        md_block0(p, out_dev, ball);
        if (p.flags & F_RESID) {
            fwd2(U0, nullptr, T(0), innerb, CNs);
            {
                ProfScope ps(prof, PS_OTHER);
                launch_permute_ab<cx<T>>(st, innerb, md_coef, H, (int64_t)Wf * CN, 1);
            }
            // (column FFT of those row spectra and the sum in one read pass: csc_fused.h)
            auto da = fused_cols_args(p.rho, false, wk);
            da.sft = md_coef;
            {
                ProfScope ps(prof, PS_SETCOEF_COLS);
                nb = (int)launch_cols_dualres<T>(st, da);
            }
            const int slots[1] = {SPORCO_AMD_OUT_S2};
            const double scales[1] = {1.0 / ((double)H * W)};
            finalize(part_f, nb, 1, 1, slots, scales, out_dev);
        }
    }

    void mdcpl_iter(const sporco_amd_admm_params &p, double *out_dev) override { md_iterate(p, out_dev, false); }
    // ConvMinL1InL2Ball (sporco/admm/cbpdn.py:1830-2060): the same iteration with block 0 projected
    // onto the l2 balls of radius p.mu (md_block0); the handle's data mask is not read
    void ball_iter(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(p.mu >= 0.0, "epsilon (params.mu) must not be negative");
        md_iterate(p, out_dev, true);
    }
    void md_iterate(const sporco_amd_admm_params &p, double *out_dev, bool ball) {
        require_ready();
        SA_REQUIRE(md_s != nullptr, "mdcpl_init must be called first");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        SA_REQUIRE(!(p.flags & (F_JOINT | F_GRADREG | F_AMS)), "flag not valid for mask decoupling");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        if (mdcpl_fused_ok(p)) md_x_pending = false;   // (X of the previous iteration is superseded)
        before_state_change();
        if (mdcpl_fused_ok(p)) {
            mdcpl_iter_fused(p, out_dev, ball);
            return;
        }
        x_written();
        xf_tiled = false;
        // (a multi-channel dictionary, Cd > 1: block 0 keeps the signal's Cd channels, block 1 and
        // the coefficient maps have one -- cbpdn.py:1565-1574; the X-step is the iterated
        // Sherman-Morrison solve with rho = 1, :1621-1626)
        const int64_t ns = (int64_t)H * W * CNs;
        const T us = (T)p.u_scale;
        T *Y1 = rv(SPORCO_AMD_VAR_Y), *U1 = rv(SPORCO_AMD_VAR_U), *X = rv(SPORCO_AMD_VAR_X);
        T *Y0 = rv(SPORCO_AMD_VAR_MY0), *U0 = rv(SPORCO_AMD_VAR_MU0);
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF), *Df = cv(SPORCO_AMD_VAR_DF);
        cx<T> *Vf = cv(SPORCO_AMD_VAR_VF), *Gf = cv(SPORCO_AMD_VAR_GF);
        // xstep: b = conj(Df) rfftn(y0 - u0 + s) + rfftn(y1 - u1); (D^H D + I) Xf = b
        // (the block-0 spectrum in the signal's place; partial 0 is the solve's own residual against it)
        {
            ProfScope ps(prof, PS_OTHER);
            launch_md_pre<T>(st, Y0, U0, md_s, sreal, us, ns);
        }
        fwd2(sreal, nullptr, T(0), innerb, CNs);
        fwd2(Y1, U1, us, Vf, P);
        const bool xr = p.flags & F_XRRS;
        int nb = generic_solve(Vf, Xf, innerb, T(1), false, xr, nullptr, -1.0);
        if (xr) finalize_solve(nb, 4, 0.0, SPORCO_AMD_OUT_RGR, out_dev);
        inv2(Xf, work_buf(), X, P);
        // block 0: AXnr = D x, relax, y0, u0
        {
            ProfScope ps(prof, PS_OTHER);
            inner_df(Xf);
        }
        inv2(innerb, innerb, sreal, CNs);
        // block 1: relax, y1 = prox_l1 (+ NonNegCoef / NoBndryCross), u1 and the sums
        const PostParams<T> pp = post_params(p, X, Y1, U1);
        {
            ProfScope ps(prof, PS_ADMM_POST);
            nb = launch_admm_post<T>(st, pp, part_b);
        }
        finalize_post(part_b, nb, 6, false, out_dev);
        md_block0(p, out_dev, ball);
        if (p.flags & F_RESID) {
            // dual residual (cbpdn.py:1814-1818): A^T u = irfftn(conj(Df) rfftn(u0)) + u1, its
            // norm through the half-spectrum Parseval sum
            fwd2(U0, nullptr, T(0), innerb, CNs);
            fwd2(U1, nullptr, T(0), Vf, P);
            {
                ProfScope ps(prof, PS_OTHER);
                if (Cd > 1) launch_mc_conj_outer<T>(st, Df, innerb, Gf, npix, Cd, N, K, false);
                else launch_conj_outer<T>(st, Df, innerb, Gf, npix, CN, K);
                launch_lincomb<T>(st, Gf, T(1), Gf, T(1), Vf, T(0), nullptr, EF);
                nb = launch_pair_stats<T>(st, Gf, nullptr, nullptr, npix, P, W, part_b);
            }
            const int slots[1] = {SPORCO_AMD_OUT_S2};
            const double scales[1] = {1.0 / ((double)H * W)};
            finalize(part_b, nb, 4, 1, slots, scales, out_dev);
        }
    }
