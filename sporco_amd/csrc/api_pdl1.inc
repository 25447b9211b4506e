// api_pdl1.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint (sporco/admm/pdcsc.py:293-701), the
// product dictionary of api_pd.inc under the l1 data fidelity of api_l1l1.inc (csc_pdl1.h).
    // The handle has C = Cb channels, as for ConvProdDictBPDN: block 1 (VAR_Y / VAR_U), X, L1Weight,
    // GradWeight and the tables of pd_setup are the handle's own.  Block 0 has the signal's Cs
    // channels, which the handle's signal-shaped arrays have not: it lives in buffers of its own,
    // owned here.  Generic transforms on every shape.
    int pl_Cs = 0;
    T *pl_s = nullptr;              // S                                     (H, W, Cs N)
    T *pl_y0 = nullptr, *pl_u0 = nullptr;
    T *pl_ax0 = nullptr;            // y0 - u0 + s on its way in, A0 x on its way out
    cx<T> *pl_z0f = nullptr;        // rfftn(y0 - u0 + s); rfftn(u0) for the dual residual  (npix, Cs N)
    cx<T> *pl_ax0f = nullptr;       // (BQ)(d . xh)                          (npix, Cs N)
    T *pl_wbuf = nullptr;           // the mask, expanded                    (H, W, Cs N)
    int pl_wave_launches = 0, pl_generic_launches = 0;

    void pdl1_release() {
        for (void *p : {(void *)pl_s, (void *)pl_y0, (void *)pl_u0, (void *)pl_ax0, (void *)pl_z0f, (void *)pl_ax0f,
                        (void *)pl_wbuf})
            if (p) (void)hipFree(p);
        pl_s = pl_y0 = pl_u0 = pl_ax0 = pl_wbuf = nullptr;
        pl_z0f = pl_ax0f = nullptr;
        pl_Cs = 0;
    }

    // The tables and signal of pd_setup, the mask (null: none; else T, expanded to (H, W, Cs, N)), and
    // block 0: created at zero by the first call, kept by a later one (setdict between two solves).
    void pdl1_setup(const double *B, const double *Q, const double *gamma, const void *S, int cs,
                    const void *mask) override {
        pd_setup(B, Q, gamma, S, cs);
        const size_t nr = (size_t)H * W * cs * N, nf = (size_t)npix * cs * N;
        if (pl_Cs != cs) {
            pdl1_release();
            pl_Cs = cs;
            for (T **p : {&pl_s, &pl_y0, &pl_u0, &pl_ax0}) SA_HIP(hipMalloc((void **)p, sizeof(T) * nr));
            SA_HIP(hipMalloc((void **)&pl_z0f, sizeof(cx<T>) * nf));
            SA_HIP(hipMalloc((void **)&pl_ax0f, sizeof(cx<T>) * nf));
            SA_HIP(hipMemsetAsync(pl_y0, 0, sizeof(T) * nr, st));
            SA_HIP(hipMemsetAsync(pl_u0, 0, sizeof(T) * nr, st));
        }
        SA_HIP(hipMemcpyAsync(pl_s, S, sizeof(T) * nr, hipMemcpyHostToDevice, st));
        if (mask) {
            if (!pl_wbuf) SA_HIP(hipMalloc((void **)&pl_wbuf, sizeof(T) * nr));
            SA_HIP(hipMemcpyAsync(pl_wbuf, mask, sizeof(T) * nr, hipMemcpyHostToDevice, st));
        } else if (pl_wbuf) {
            sync();
            SA_HIP(hipFree(pl_wbuf));
            pl_wbuf = nullptr;
        }
        sync();      // the host buffers may be released after return
    }

    // which: 0 = y0, 1 = u0 (H, W, Cs, N); to_device: upload, else download
    void pdl1_block0(int which, bool to_device, void *host) override {
        SA_REQUIRE(pl_Cs > 0, "pdl1_block0 without pdl1_setup");
        SA_REQUIRE(which == 0 || which == 1, "pdl1_block0: 0 (y0) or 1 (u0)");
        T *dev = which == 0 ? pl_y0 : pl_u0;
        const size_t nb = sizeof(T) * (size_t)H * W * pl_Cs * N;
        if (to_device) SA_HIP(hipMemcpyAsync(dev, host, nb, hipMemcpyHostToDevice, st));
        else SA_HIP(hipMemcpyAsync(host, dev, nb, hipMemcpyDeviceToHost, st));
        sync();
    }

    // One iteration (pdcsc.py:509-540 and the steps of ConvL1L1Grd, cbpdn.py:2716-2749).  F_JOINT: block
    // 1 is prox_sl1l2(., 0, lmbda / rho) over the channel axis (pdcsc.py:681-692).
    void pdl1_iter(const sporco_amd_admm_params &p, double *out_dev) override {
        require_ready();
        SA_REQUIRE(pd_active && pl_Cs == pd_Cs && pl_Cs > 0, "pdl1_iter without pdl1_setup");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        SA_REQUIRE(p.mu >= 0.0, "mu must not be negative");
        SA_REQUIRE(!(p.flags & F_AMS), "flag not valid for ConvProdDictL1L1Grd");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        before_state_change();
        x_written();
        xf_tiled = false;
        const int64_t csn = (int64_t)pl_Cs * N, ns = (int64_t)H * W * csn;
        const T us = (T)p.u_scale;
        const bool want_dual = p.flags & F_RESID, joint = p.flags & F_JOINT;
        T *Y1 = rv(SPORCO_AMD_VAR_Y), *U1 = rv(SPORCO_AMD_VAR_U), *X = rv(SPORCO_AMD_VAR_X);
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF), *Df = cv(SPORCO_AMD_VAR_DF), *Vf = cv(SPORCO_AMD_VAR_VF);
        // x step
        {
            ProfScope ps(prof, PS_OTHER);
            launch_md_pre<T>(st, pl_y0, pl_u0, pl_s, pl_ax0, us, ns);
        }
        fwd2(pl_ax0, nullptr, T(0), pl_z0f, csn);
        fwd2(Y1, U1, us, Vf, P);
        Pdl1SolveArgs<T> a;
        a.z0f = pl_z0f;
        a.z1f = Vf;
        a.xf = Xf;
        a.ax0f = pl_ax0f;
        a.df = Df;
        a.grad = grad_term(p.mu / p.rho);
        a.tab = pd_tables();
        a.npix = npix;
        a.Cb = C;
        a.Cs = pl_Cs;
        a.N = N;
        a.K = K;
        a.W = W;
        a.want_obj = (p.flags & F_OBJ) ? 1 : 0;
        a.want_xrrs = (p.flags & F_XRRS) ? 1 : 0;
        a.force_generic = sw.pdl1_generic ? 1 : 0;
        a.partials = part_a;
        int nb;
        bool wave = false;
        {
            ProfScope ps(prof, PS_PDL1_SOLVE);
            nb = launch_pdl1_solve<T>(st, a, &wave);
        }
        ++(wave ? pl_wave_launches : pl_generic_launches);
        if (a.want_obj || a.want_xrrs) {
            const int slots[4] = {SPORCO_AMD_OUT_RGRX, SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2,
                                  SPORCO_AMD_OUT_XRRS_B2};
            const double scales[4] = {1.0 / ((double)H * W), 1.0, 1.0, 1.0};
            finalize(part_a, nb, 4, 4, slots, scales, out_dev);
        }
        inv2(Xf, work_buf(), X, P);
        inv2(pl_ax0f, pl_ax0f, pl_ax0, csn);
        // block 1: relax, y1 = prox (+ NonNegCoef / NoBndryCross), u1, the sums
        // (joint: lmbda / rho is the l2,1 threshold, the l1 threshold zero and L1Weight ignored; the
        // handle's l2,1 weight array is never this class's)
        PostParams<T> pp = post_params(p, X, Y1, U1);
        if (joint) {
            std::swap(pp.thr, pp.thr21);
            pp.wl1 = Weight<T>();
        }
        pp.wl21 = Weight<T>();
        {
            ProfScope ps(prof, PS_ADMM_POST);
            nb = launch_admm_post<T>(st, pp, part_b);
        }
        finalize_post(part_b, nb, joint ? 7 : 6, false, out_dev);
        // block 0
        L1Y0Args<T> ya;
        ya.ax0nr = pl_ax0;
        ya.y0 = pl_y0;
        ya.u0 = pl_u0;
        ya.s = pl_s;
        ya.dy0 = nullptr;
        if (pl_wbuf) {
            ya.w.ptr = pl_wbuf;
            ya.w.stride[0] = (int64_t)W * csn;
            ya.w.stride[1] = csn;
            ya.w.stride[2] = N;
            ya.w.stride[3] = 1;
            ya.w.stride[4] = 0;
        }
        ya.rho = (T)p.rho;
        ya.rlx = (T)p.rlx;
        ya.us = us;
        ya.geval_y = (p.flags & F_GEVAL_Y) ? 1 : 0;
        ya.H = H;
        ya.W = W;
        ya.C = pl_Cs;
        ya.N = N;
        {
            ProfScope ps(prof, PS_L1L1_Y0STEP);
            nb = launch_l1l1_y0step<T>(st, ya, part_a);
        }
        {
            const int slots[5] = {SPORCO_AMD_OUT_R02, SPORCO_AMD_OUT_RGR, SPORCO_AMD_OUT_CNSTR, SPORCO_AMD_OUT_CGIT,
                                  SPORCO_AMD_OUT_DFID};
            const double scales[5] = {1, 1, 1, 1, 1};
            finalize(part_a, nb, 5, 5, slots, scales, out_dev);
        }
        if (want_dual) {
            // s = rho ||A^T U|| at the new U (pdcsc.py:568-571): two forward transforms and one
            // read-only pass; sn = rho ||U|| comes from the sums of the block steps
            fwd2(pl_u0, nullptr, T(0), pl_z0f, csn);
            fwd2(U1, nullptr, T(0), Vf, P);
            Pdl1DualArgs<T> da;
            da.df = Df;
            da.u0f = pl_z0f;
            da.u1f = Vf;
            da.b = pd_tables().b;
            da.npix = npix;
            da.Cb = C;
            da.Cs = pl_Cs;
            da.N = N;
            da.K = K;
            da.W = W;
            da.partials = part_b;
            {
                ProfScope ps(prof, PS_PDL1_DUAL);
                nb = launch_pdl1_dual<T>(st, da);
            }
            const int slots[1] = {SPORCO_AMD_OUT_S2};
            const double scales[1] = {1.0 / ((double)H * W)};
            finalize(part_b, nb, 2, 1, slots, scales, out_dev);
        }
    }
