// api_admm.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ADMM ConvBPDN family: fused and staged iterations.
    // ---- ADMM --------------------------------------------------------------------
    // The tables of the iterated Sherman-Morrison solve (multi-channel dictionary): allocated on
    // first use, rebuilt when they were built for another system than the one asked for.  The
    // system is (rho, the gradient diagonal gt); mu_key names the diagonal -- the mu it was built
    // with, -1 for none -- so that a handle serving several solver kinds in turn (a gradient-
    // regularised solve, then a mask-decoupled one with rho = 1) never reuses the other kind's
    // tables.  A new dictionary or GradWeight clears ism_valid.  (Without gt the kernel does not
    // read W.)
    void ism_tables(double rho, const GradTerm<T> *gt, double mu_key) {
        if (!ism_gam) {
            SA_HIP(hipMalloc((void **)&ism_gam, sizeof(cx<T>) * npix * Cd * K));
            SA_HIP(hipMalloc((void **)&ism_del, sizeof(cx<T>) * npix * Cd));
            SA_HIP(hipMalloc((void **)&ism_mm, sizeof(cx<T>) * npix * Cd * Cd));
        }
        if (ism_valid && ism_rho == rho && ism_mu == mu_key) return;
        ProfScope ps(prof, PS_OTHER);
        launch_ism_setup<T>(st, cv(SPORCO_AMD_VAR_DF), ism_gam, ism_del, ism_mm, npix, Cd, K, (T)rho, gt, W);
        ism_valid = true;
        ism_rho = rho;
        ism_mu = mu_key;
    }

    // The generic chain's solve of (D^H D + rho I [+ gt]) xf = conj(Df) sf + rho b in the natural
    // layout: Sherman-Morrison, or its iterated form for a multi-channel dictionary (cbpdn.py:277-279;
    // with gt the identity term is the diagonal mu wg GHGf + rho, :1181-1184).  Partials to part_a
    // (finalize_solve); returns the number of blocks that wrote them.
    int generic_solve(const cx<T> *b, cx<T> *xf, const cx<T> *sf, T rho, bool obj, bool xr,
                      const GradTerm<T> *gt, double mu_key) {
        if (Cd > 1) ism_tables((double)rho, gt, mu_key);
        ProfScope ps(prof, PS_SM_SOLVE);
        if (Cd > 1)
            return launch_ism_solve<T>(st, b, xf, cv(SPORCO_AMD_VAR_DF), sf, ism_gam, ism_del, ism_mm, rho, npix,
                                       Cd, N, K, W, obj, xr, part_a, gt);
        return launch_sm_solve<T>(st, b, xf, cv(SPORCO_AMD_VAR_DF), sf, gram, rho, npix, CN, K, W, obj, xr, part_a,
                                  gt);
    }

    // The column pass of the generic chain as one kernel: column transform, Sherman-Morrison solve
    // and inverse column transform of a (wf, cn) tile in LDS (fft.h fft_cols_sm), two passes over
    // the spectrum instead of six; the data fidelity -> out_dev.  The Xf buffer is left holding the
    // column-inverse-transformed solution (the caller marks it xf_tiled).
    void run_cols_sm(const sporco_amd_admm_params &p, bool obj, double *out_dev) {
        if (!part_cs) SA_HIP(hipMalloc((void **)&part_cs, sizeof(double) * (int64_t)Wf * CN));
        int64_t nt;
        {
            ProfScope ps(prof, PS_SM_SOLVE);
            nt = fft_cols_sm<T>(st, planH, cv(SPORCO_AMD_VAR_XF), cv(SPORCO_AMD_VAR_DF), cv(SPORCO_AMD_VAR_SF), gram,
                                (T)p.rho, Wf, CN, K, W, obj, part_cs, sw.cols_sm_force_slab, &cols_sm_form);
        }
        if (obj) {
            const int slots[1] = {SPORCO_AMD_OUT_DFID};
            const double scales[1] = {1.0 / ((double)H * W)};
            finalize(part_cs, (int)nt, 1, 1, slots, scales, out_dev);
        }
    }

    // X-step: Xf = SM(rfftn(Y - s U)), X = irfftn(Xf); objective / check sums -> out_dev
    // (gv: the iterate as the single array V = AX + U, produced with the threshold gv_thr_in --
    // the generic row transform derives Y - s U from it; admm_iter)
    void xstep_impl(const sporco_amd_admm_params &p, double *out_dev, const T *gv = nullptr,
                    T gv_thr_in = T(0)) {
        require_ready();
        x_written();
        t_ready = false;
        const VformIn<T> vfi{gv_thr_in, (bool)(p.flags & F_NONNEG)};
        const VformIn<T> *vf = gv ? &vfi : nullptr;
        const T *Y = gv ? gv : rv(SPORCO_AMD_VAR_Y), *U = gv ? nullptr : rv(SPORCO_AMD_VAR_U);
        T *X = rv(SPORCO_AMD_VAR_X);
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF);
        const bool gradreg = p.flags & F_GRADREG;
        if (cplx) {
            // complex signal / dictionary: real transforms of the channel pairs around the paired
            // solve (ck_admm.hip sm_cplx_kernel)
            SA_REQUIRE(!(p.flags & (F_XRRS | F_GRADREG)),
                       "complex mode: no LinSolveCheck, no gradient term");
            xf_tiled = false;
            fwd2(Y, U, (T)p.u_scale, Xf, P, vf);
            const bool objc = (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y);
            int nbc;
            {
                ProfScope ps(prof, PS_SM_SOLVE);
                nbc = launch_sm_cplx<T>(st, Xf, cv(SPORCO_AMD_VAR_DF), df_im, cv(SPORCO_AMD_VAR_SF), npix,
                                        C / 2, N, K, (T)p.rho, W, objc, part_a);
            }
            if (objc) {
                const int slots[1] = {SPORCO_AMD_OUT_DFID};
                const double scales[1] = {1.0 / ((double)H * W)};
                finalize(part_a, nbc, 1, 1, slots, scales, out_dev);
            }
            inv2(Xf, work_buf(), X, P);
            return;
        }
        if ((fused || (fused_slabs && rows_ok) || (fused_mc && rows_ok)) &&
            !(p.flags & F_XRRS) && mr_ok(p)) {
            // rows -> [column FFT, Sherman-Morrison, column IFFT] in registers -> rows,
            // through the tile-major intermediate T[wf][cn][h][k] held in the Xf buffer
            const int64_t tline = (int64_t)CN * H * K, tgrp = (int64_t)H * K;
            if (rows_ok) {
                // register-resident row passes around it (ConvBPDNJoint, staged callers)
                launch_rows_fwd_on(Y, U, (T)p.u_scale);
                run_fused_cols(p, out_dev);
                rows_inverse_to(X);
                return;
            }
            {
                ProfScope ps(prof, PS_FFT_R2C);
                fft_r2c<T>(st, planW, Y, U, (T)p.u_scale, Xf, H, P, (int64_t)W * P, P, K, tline, K,
                           tgrp, 0, vf);
            }
            run_fused_cols(p, out_dev);
            {
                ProfScope ps(prof, PS_FFT_C2R);
                fft_c2r<T>(st, planW, Xf, X, H, P, K, tline, (int64_t)W * P, P,
                           T(1.0 / ((double)H * (double)W)), K, tgrp);
            }
            return;
        }
        xf_tiled = false;
        const bool obj = (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y);
        const bool xr = p.flags & F_XRRS;
        if (cols_sm_ok(p)) {
            // the one-kernel column pass between the two row passes
            {
                ProfScope ps(prof, PS_FFT_R2C);
                fft_r2c<T>(st, planW, Y, U, (T)p.u_scale, Xf, H, P, (int64_t)W * P, P, (int64_t)Wf * P, P,
                           0, 0, 0, vf);
            }
            run_cols_sm(p, obj, out_dev);
            xf_tiled = true;       // (a reader of VAR_XF gets rfftn(X))
            {
                ProfScope ps(prof, PS_FFT_C2R);
                fft_c2r<T>(st, planW, Xf, X, H, P, (int64_t)Wf * P, P, (int64_t)W * P, P,
                           T(1.0 / ((double)H * (double)W)));
            }
            return;
        }
        // (ConvBPDNGradReg: the gradient term; AddMaskSim and ConvBPDNJoint differ in the y step only)
        fwd2(Y, U, (T)p.u_scale, Xf, P, vf);
        GradTerm<T> gt;
        if (gradreg) gt = grad_term(p.mu);
        const int nb = generic_solve(Xf, Xf, cv(SPORCO_AMD_VAR_SF), (T)p.rho, obj, xr, gradreg ? &gt : nullptr,
                                     gradreg ? p.mu : -1.0);
        if (obj || xr) finalize_solve(nb, gradreg ? 5 : 4, 1.0 / ((double)H * W), SPORCO_AMD_OUT_RGR, out_dev);
        inv2(Xf, work_buf(), X, P);
    }

    // the generic X-step's column pass as one LDS-resident kernel (fft.h fft_cols_sm): single-
    // channel dictionary, plain system (no gradient term, no LinSolveCheck residual), the
    // epilogue not deferred into the row pass
    double *part_cs = nullptr;
    ColsSmForm cols_sm_form;      // what the last fft_cols_sm call launched (threads 0: none yet)
    bool cols_sm_ok(const sporco_amd_admm_params &p) const {
        return Cd == 1 && depth == 1 && !(p.flags & (F_GRADREG | F_XRRS)) && !sw.no_cols_sm &&
               fft_cols_sm_supported<T>(planH, K, sw.cols_sm_force_slab);
    }

    // data fidelity evaluated at Y (fEvalX False / AuxVarObj, cbpdn.py:315-321)
    // innerb(npix, Cs, N) = sum_k Df * vf   (linalg.inner over the filter axis)
    void inner_df(const cx<T> *vf) {
        if (cplx)
            launch_inner_cplx<T>(st, cv(SPORCO_AMD_VAR_DF), df_im, vf, innerb, npix, C / 2, N, K);
        else if (Cd > 1)
            launch_mc_inner<T>(st, cv(SPORCO_AMD_VAR_DF), vf, innerb, npix, Cd, N, K);
        else
            launch_inner<T>(st, cv(SPORCO_AMD_VAR_DF), vf, innerb, npix, CN, K);
    }

    void dfid_at(const T *V, double *out_dev, const sporco_amd_admm_params *gp = nullptr) {
        cx<T> *wk = work_buf();
        fwd2(V, nullptr, T(0), wk, P);
        if (gp && (gp->flags & F_GRADREG)) {
            // the gradient term follows the data-fidelity variable (cbpdn.py:1209-1213)
            int nbg;
            {
                ProfScope ps(prof, PS_OTHER);
                nbg = launch_grad_norm<T>(st, wk, grad_term(gp->mu), npix, CN, K, W, part_a);
            }
            const int gslots[1] = {SPORCO_AMD_OUT_RGR};
            const double gscales[1] = {1.0 / ((double)H * W)};
            finalize(part_a, nbg, 1, 1, gslots, gscales, out_dev);
        }
        {
            ProfScope ps(prof, PS_OTHER);
            inner_df(wk);
        }
        int nb;
        {
            ProfScope ps(prof, PS_OTHER);
            nb = launch_rfl2norm2<T>(st, innerb, cv(SPORCO_AMD_VAR_SF), npix, CNs, W, part_a);
        }
        const int slots[1] = {SPORCO_AMD_OUT_DFID};
        const double scales[1] = {1.0 / ((double)H * W)};
        finalize(part_a, nb, 1, 1, slots, scales, out_dev);
    }

    // 64 < K <= 64 + kTailMax: the gradient-regularised column pass is available too
    bool grad_tail_ok() const { return tail_mode; }

    // the impulse filters AddMaskSim appended: one, or one per channel of a multi-channel
    // dictionary (cbpdn.py:2339-2346); they are the last filters the caller passed
    int ams_n() const { return Cd > 1 ? Cd : 1; }
    int ams_k0() const { return Ku - ams_n(); }

    // the AddMaskSim mask, when the call asks for it (F_AMS)
    Weight<T> ams_of(const sporco_amd_admm_params &p) const {
        if (!(p.flags & F_AMS)) return Weight<T>();
        if (!wams.ptr) throw Error(SPORCO_AMD_ESTATE, "FLAG_AMS without a mask (set_ams_mask)");
        return wams;
    }

    // the same mask, one bit per pixel in the row kernel's order (built on first use)
    const uint32_t *ams_bits_of(const sporco_amd_admm_params &p) {
        if (!(p.flags & F_AMS)) return nullptr;
        const Weight<T> m = ams_of(p);
        if (!ams_bits_valid) {
            if (!ams_bits)
                SA_HIP(hipMalloc((void **)&ams_bits,
                                 sizeof(uint32_t) * (int64_t)H * CN * (rows_mr_width(W) ? 16 : W / 32)));
            ProfScope ps(prof, PS_OTHER);
            launch_ams_pack<T>(st, m, ams_bits, H, W, C, N);
            ams_bits_valid = true;
        }
        return ams_bits;
    }

    // ConvBPDNJoint inside the row epilogue (csc_rows.h): scalar weights, no NoBndryCross /
    // AddMaskSim, C <= 4 channels, K a multiple of 32, single-channel dictionary
    bool joint_rows_ok(const sporco_amd_admm_params &p) const {
        return rows_ok && !fused_mc && rows_joint_supported<T>(W, C, K) && !wl1.ptr && !wl21.ptr &&
               !(p.flags & (F_NOBNDRY | F_AMS | F_KEEP_X | F_GRADREG));
    }

    // The generic chain's iterate after an iteration with the parameters p: live, it is V in the
    // buffer of vars[U] (no buffer of its own in the record, no previous V); the threshold and
    // NonNegCoef are kept either way, for the next iteration's choice
    void commit_generic_v(const sporco_amd_admm_params &p, bool live) {
        it.form = live ? IterForm::GenericV : IterForm::YU;
        it.cur = held_v(p, nullptr, (T)(p.lmbda / p.rho), T(0));
    }

    void admm_iter(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(depth == 1 || !(p.flags & (F_NOBNDRY | F_GRADREG | F_AMS)),
                   "volume handle: no NoBndryCross, gradient term or AddMaskSim (their kernels know two axes)");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        // (a negative lambda -- meaningless, but the reference's soft threshold is defined for it --
        // goes to the generic chain: the row kernels clamp with a threshold known to be >= 0)
        if (!cplx && rows_ok && mr_ok(p) && !(p.flags & F_XRRS) && (!(p.flags & F_JOINT) || joint_rows_ok(p)) &&
            (fused || fused_slabs || !(p.flags & F_GRADREG)) && p.lmbda >= 0.0 && p.rho > 0.0 &&
            !(Cd > 1 && (p.flags & (F_GRADREG | F_AMS | F_JOINT)))) {
            // (a multi-channel dictionary under ConvBPDNGradReg / AddMaskSim / ConvBPDNJoint:
            // the generic chain -- the register kernels know one impulse slice and no diagonal)
            admm_iter_fused(p, out_dev);
            return;
        }
        // Single-array state of the generic chain: from the second iteration in a row with no
        // host access to the iterates in between, the epilogue stores V' = AX + U alone (in the
        // buffer of U) and the row transform and the next epilogue derive (Y, U) from it:
        // thirteen passes over an array of the coefficients' size instead of sixteen.
        const bool gnn = p.flags & F_NONNEG;
        const bool gv_in = it.form == IterForm::GenericV && gvform_ok(p) && it.cur.nonneg == gnn;
        const bool gv_out = gvform_ok(p) && (gv_in || touch_epoch == gen_epoch);
        // (float64: measured +5 ... 7 % there -- 256 x 256, K = 32: 2107 -> 2217 it/s --, -2 ... +3 % in
        // float32, whose three separate kernels are not bound by the passes it saves:
        // profiles/r05v_generic_fused_rows.jsonl)
        if (std::is_same<T, double>::value && gv_in && gv_out && cols_sm_ok(p) && !cplx &&
            fft_c2r_vpost_supported<T>(P)) {
            admm_iter_generic_fused(p, out_dev);
            return;
        }
        if (gv_in) {
            ++touch_epoch;
            pgm_rx_count = 0;
            t_ready = false;
        } else {
            before_state_change();
        }
        T *const ybuf = gv_in ? static_cast<T *>(vars[SPORCO_AMD_VAR_Y]) : rv(SPORCO_AMD_VAR_Y);
        T *const ubuf = gv_in ? static_cast<T *>(vars[SPORCO_AMD_VAR_U]) : rv(SPORCO_AMD_VAR_U);
        xstep_impl(p, out_dev, gv_in ? ubuf : nullptr, it.cur.thr);
        PostParams<T> pp = post_params(p, rv(SPORCO_AMD_VAR_X), ybuf, ubuf);
        pp.v_in = gv_in ? ubuf : nullptr;
        pp.v_out = gv_out ? ubuf : nullptr;
        pp.thr_prev = it.cur.thr;
        if (p.flags & F_JOINT) pp.thr21 = (T)(p.mu / p.rho);
        commit_generic_v(p, gv_out);
        {
            x_written();
            int nb;
            {
                ProfScope ps(prof, PS_ADMM_POST);
                nb = launch_admm_post<T>(st, pp, part_b);
            }
            finalize_post(part_b, nb, 7, true, out_dev);
        }
        if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) dfid_at(rv(SPORCO_AMD_VAR_Y), out_dev, &p);
        gen_epoch = touch_epoch;
    }

    // The generic chain from the second iteration of a run in the single-array state, where the
    // column pass is the one-kernel form: r2c row pass (skipped when the previous iteration emitted
    // the spectrum and rho stayed), column pass, and ONE kernel for the c2r row pass, the epilogue
    // and -- rho stable for two updates -- the next iteration's row spectrum (fft.h fft_c2r_vpost):
    // 7 X-sized passes, 6 with the emission, instead of 9.  X exists on demand (materialize_x).
    void admm_iter_generic_fused(const sporco_amd_admm_params &p, double *out_dev) {
        ++touch_epoch;
        pgm_rx_count = 0;
        x_written();       // (a pending X of the previous iteration is superseded)
        T *const vbuf = static_cast<T *>(vars[SPORCO_AMD_VAR_U]);
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF);
        if (!(t_ready && p.u_scale == 1.0)) {
            const VformIn<T> vfi{it.cur.thr, (bool)(p.flags & F_NONNEG)};
            ProfScope ps(prof, PS_FFT_R2C);
            fft_r2c<T>(st, planW, vbuf, nullptr, (T)p.u_scale, Xf, H, P, (int64_t)W * P, P, (int64_t)Wf * P, P,
                       0, 0, 0, &vfi);
        }
        t_ready = false;
        run_cols_sm(p, (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y), out_dev);
        stable_run = p.u_scale == 1.0 ? stable_run + 1 : 0;
        const bool emit = stable_run >= 2 && !sw.no_speculation;
        if (emit && !gemit) big_alloc((void **)&gemit, var_alloc_bytes(SPORCO_AMD_VAR_XF));
        const int64_t nblk = fft_c2r_vpost_blocks<T>(planW, H, P);
        if (nblk > part_vpost_cap) {
            if (part_vpost) {
                sync();
                SA_HIP(hipFree(part_vpost));
            }
            SA_HIP(hipMalloc((void **)&part_vpost, sizeof(double) * 8 * nblk));
            part_vpost_cap = nblk;
        }
        // (gvform_ok: no weight array, no F_JOINT, no F_AMS on this path)
        PostParams<T> pp = post_params(p, nullptr, nullptr, nullptr);
        pp.v_in = vbuf;
        pp.v_out = vbuf;
        pp.thr_prev = it.cur.thr;
        int64_t nb;
        {
            ProfScope ps(prof, emit ? PS_C2R_VPOST_EMIT : PS_C2R_VPOST);
            nb = fft_c2r_vpost<T>(st, planW, Xf, H, P, (int64_t)Wf * P, P, T(1.0 / ((double)H * (double)W)), pp,
                                  emit ? gemit : nullptr, (int64_t)Wf * P, P, part_vpost);
        }
        finalize_post(part_vpost, (int)nb, 7, true, out_dev);
        commit_generic_v(p, true);
        // X of this iteration: one c2r row pass of the column pass's output away
        x_invalid = p.flags & F_NO_X;
        md_x_pending = !x_invalid;
        gx_buf = Xf;
        xf_tiled = true;       // (the Xf buffer does not hold rfftn(X): a reader gets it rebuilt from X)
        if (emit) {
            std::swap(vars[SPORCO_AMD_VAR_XF], reinterpret_cast<void *&>(gemit));
            gx_buf = gemit;    // (the buffers traded places: the column output is in gemit now)
            t_ready = true;
        }
        gen_epoch = touch_epoch;
    }

    void admm_xstep(const sporco_amd_admm_params &p, double *out_dev) override {
        before_state_change();
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        xstep_impl(p, out_dev);
    }

    void admm_relax(double rlx) override {
        before_read(SPORCO_AMD_VAR_X);
        ProfScope ps(prof, PS_OTHER);
        launch_relax<T>(st, rv(SPORCO_AMD_VAR_X), rv(SPORCO_AMD_VAR_Y), rv(SPORCO_AMD_VAR_AX), (T)rlx,
                        E);
    }

    void admm_ystep(const sporco_amd_admm_params &p) override {
        ProfScope ps(prof, PS_OTHER);
        launch_ystep<T>(st, rv(SPORCO_AMD_VAR_AX), rv(SPORCO_AMD_VAR_U), rv(SPORCO_AMD_VAR_Y),
                        (T)(p.lmbda / p.rho), (T)(p.mu / p.rho), (T)p.u_scale, p.flags, d5(), p.dH,
                        p.dW, wl1, wl21, ams_of(p), ams_k0(), ams_n());
    }

    void admm_ustep(const sporco_amd_admm_params &p) override {
        ProfScope ps(prof, PS_OTHER);
        launch_ustep<T>(st, rv(SPORCO_AMD_VAR_AX), rv(SPORCO_AMD_VAR_Y), rv(SPORCO_AMD_VAR_U),
                        (T)p.u_scale, E);
    }

    void admm_stats(const sporco_amd_admm_params &p, double *out_dev) override {
        before_read(SPORCO_AMD_VAR_X);
        // keeps the xstep sums already in out_dev; fills the residual/regulariser slots
        int nb;
        {
            ProfScope ps(prof, PS_OTHER);
            nb = launch_admm_stats<T>(st, rv(SPORCO_AMD_VAR_X), rv(SPORCO_AMD_VAR_Y),
                                      rv(SPORCO_AMD_VAR_YPREV), rv(SPORCO_AMD_VAR_U), p.flags, d5(),
                                      wl1, wl21, (p.flags & F_AMS) ? ams_k0() : -1, part_b,
                                      ams_n());
        }
        finalize_post(part_b, nb, 7, true, out_dev);
        if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) dfid_at(rv(SPORCO_AMD_VAR_Y), out_dev, &p);
    }

    void scale_u(double s) override {
        ProfScope ps(prof, PS_OTHER);
        launch_scale<T>(st, rv(SPORCO_AMD_VAR_U), (T)s, E);
    }

    // irfftn(sum_k Df rfftn(var)) into sreal, copied out to the host or to device memory
    void reconstruct_to(int var, void *dst, hipMemcpyKind kind) {
        require_ready();
        SA_REQUIRE(!var_is_complex(var), "reconstruct needs a real state variable");
        before_read(var);
        cx<T> *wk = work_buf();
        fwd2(rv(var), nullptr, T(0), wk, P);
        {
            ProfScope ps(prof, PS_OTHER);
            inner_df(wk);
        }
        inv2(innerb, innerb, sreal, CNs);
        SA_HIP(hipMemcpyAsync(dst, sreal, sizeof(T) * (int64_t)H * W * CNs, kind, st));
        sync();
    }
    void reconstruct(int var, void *dst) override { reconstruct_to(var, dst, hipMemcpyDeviceToHost); }
    void reconstruct_dev(int var, void *dst_dev) override { reconstruct_to(var, dst_dev, hipMemcpyDeviceToDevice); }

    void dhs_absmax(double *out_host) override {
        require_ready();
        int nb;
        {
            ProfScope ps(prof, PS_OTHER);
            nb = Cd > 1 ? launch_mc_dhs_absmax<T>(st, cv(SPORCO_AMD_VAR_DF), cv(SPORCO_AMD_VAR_SF),
                                                   npix, Cd, N, K, part_a)
                        : launch_dhs_absmax<T>(st, cv(SPORCO_AMD_VAR_DF), cv(SPORCO_AMD_VAR_SF), npix,
                                               CN, K, part_a);
        }
        const int slots[1] = {0};
        const double scales[1] = {1.0};
        SA_HIP(hipMemsetAsync(out_dev_own, 0, sizeof(double) * kOutSlots, st));
        finalize(part_a, nb, 1, 1, slots, scales, out_dev_own, true);
        double tmp[kOutSlots];
        read_out(out_dev_own, tmp);
        *out_host = std::sqrt(tmp[0]);
    }
