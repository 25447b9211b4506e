// api_pd.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvProdDictBPDN / ConvProdDictBPDNJoint (sporco/admm/pdcsc.py:28-287), sparse coding
// with a product dictionary D (x) B (csc_pd.h).
    // The handle has C = Cb channels -- those of the coefficient maps -- and a single-channel
    // dictionary; its own signal slot holds the mixed signal S (B Q), so VAR_SF is what the solve
    // multiplies by conj(Df).  Y, U, X, the weights, the y step, the u step and admm_stats are the
    // handle's own.  Beside them: the tables and the spectrum of the Cs-channel signal itself.  All
    // K-map transforms are the generic chain's (fwd2 / inv2, natural layout) on every handle.
    bool pd_active = false;
    int pd_Cs = 0;
    T *pd_tab = nullptr;            // B Q (Cs Cb), Q (Cb Cb), Gamma (Cb), B (Cs Cb)
    cx<T> *pd_sf = nullptr;         // rfftn(S)                              (npix, Cs N)
    cx<T> *pd_rf = nullptr;         // reconstruction spectrum               (npix, Cs N)
    T *pd_sreal = nullptr;          // S on its way in, the reconstruction on its way out (H, W, Cs N)
    int pd_wave_launches = 0, pd_generic_launches = 0;

    void pd_release() {
        for (void *p : {(void *)pd_tab, (void *)pd_sf, (void *)pd_rf, (void *)pd_sreal})
            if (p) (void)hipFree(p);
        pd_tab = pd_sreal = nullptr;
        pd_sf = pd_rf = nullptr;
        pd_active = false;
    }

    PdTables<T> pd_tables() const {
        PdTables<T> t;
        t.bq = pd_tab;
        t.q = t.bq + (size_t)pd_Cs * C;
        t.gamma = t.q + (size_t)C * C;
        t.b = t.gamma + C;
        return t;
    }

    void pd_setup(const double *B, const double *Q, const double *gamma, const void *S, int cs) override {
        SA_REQUIRE(Cd == 1 && depth == 1 && !cplx, "product dictionary: single-channel real dictionary, no volume handle");
        SA_REQUIRE(C <= kPdMaxCb, "product dictionary: at most 16 columns in B (channels of the coefficient maps)");
        SA_REQUIRE(cs >= 1, "product dictionary: the signal has at least one channel");
        before_state_change();
        sync();
        pd_release();
        pd_Cs = cs;
        const size_t nt = (size_t)2 * cs * C + (size_t)C * C + C;
        std::vector<T> tab(nt);
        T *bq = tab.data(), *q = bq + (size_t)cs * C, *gm = q + (size_t)C * C, *b = gm + C;
        for (int i = 0; i < cs; ++i)
            for (int j = 0; j < C; ++j) {
                double s = 0.0;
                for (int l = 0; l < C; ++l) s += B[i * C + l] * Q[l * C + j];
                bq[i * C + j] = (T)s;
                b[i * C + j] = (T)B[i * C + j];
            }
        for (int i = 0; i < C * C; ++i) q[i] = (T)Q[i];
        for (int i = 0; i < C; ++i) gm[i] = (T)gamma[i];
        const size_t csn = (size_t)cs * N;
        SA_HIP(hipMalloc((void **)&pd_tab, sizeof(T) * nt));
        SA_HIP(hipMalloc((void **)&pd_sf, sizeof(cx<T>) * (size_t)npix * csn));
        SA_HIP(hipMalloc((void **)&pd_rf, sizeof(cx<T>) * (size_t)npix * csn));
        SA_HIP(hipMalloc((void **)&pd_sreal, sizeof(T) * (size_t)H * W * csn));
        SA_HIP(hipMemcpy(pd_tab, tab.data(), sizeof(T) * nt, hipMemcpyHostToDevice));
        SA_HIP(hipMemcpyAsync(pd_sreal, S, sizeof(T) * (size_t)H * W * csn, hipMemcpyHostToDevice, st));
        fwd2(pd_sreal, nullptr, T(0), pd_sf, (int64_t)csn);
        sync();      // the host buffer may be released after return
        pd_active = true;
    }

    // zf = rfftn(Y - us U), the eigen-channel rank-one solve (csc_pd.h; pdcsc.py:137-159), X = irfftn(Xf)
    void pd_xstep(const sporco_amd_admm_params &p, double *out_dev) override {
        SA_REQUIRE(pd_active, "pd_xstep without pd_setup");
        SA_REQUIRE(p.rho > 0.0, "pd_xstep: rho > 0");
        require_ready();
        before_state_change();
        x_written();
        xf_tiled = false;
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        cx<T> *zf = work_buf(), *Xf = cv(SPORCO_AMD_VAR_XF);
        fwd2(rv(SPORCO_AMD_VAR_Y), rv(SPORCO_AMD_VAR_U), (T)p.u_scale, zf, P);
        PdSolveArgs<T> a;
        a.zf = zf;
        a.xf = Xf;
        a.df = cv(SPORCO_AMD_VAR_DF);
        a.shf = cv(SPORCO_AMD_VAR_SF);
        a.sf = pd_sf;
        a.gram = gram;
        a.tab = pd_tables();
        a.rho = (T)p.rho;
        a.npix = npix;
        a.Cb = C;
        a.Cs = pd_Cs;
        a.N = N;
        a.K = K;
        a.W = W;
        a.want_obj = ((p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y)) ? 1 : 0;
        a.want_xrrs = (p.flags & F_XRRS) ? 1 : 0;
        a.partials = part_a;
        int nb;
        bool wave = false;
        {
            ProfScope ps(prof, PS_PD_SOLVE);
            nb = launch_pd_solve<T>(st, a, &wave);
        }
        ++(wave ? pd_wave_launches : pd_generic_launches);
        if (a.want_obj || a.want_xrrs) finalize_solve(nb, 4, 1.0 / ((double)H * W), SPORCO_AMD_OUT_RGR, out_dev);
        inv2(Xf, zf, rv(SPORCO_AMD_VAR_X), P);
    }

    // rf (may be null) = B sum_m Df_m rfftn(var)_m; with `resid` the Parseval-weighted |rf - Sf|^2
    int pd_recon_of(int var, cx<T> *rf, bool resid) {
        SA_REQUIRE(pd_active, "product dictionary call without pd_setup");
        require_ready();
        SA_REQUIRE(!var_is_complex(var), "a real state variable is needed");
        before_read(var);
        cx<T> *wk = work_buf();
        fwd2(rv(var), nullptr, T(0), wk, P);
        PdReconArgs<T> a;
        a.xf = wk;
        a.df = cv(SPORCO_AMD_VAR_DF);
        a.sf = resid ? pd_sf : nullptr;
        a.rf = rf;
        a.tab = pd_tables();
        a.npix = npix;
        a.Cb = C;
        a.Cs = pd_Cs;
        a.N = N;
        a.K = K;
        a.W = W;
        a.partials = part_a;
        ProfScope ps(prof, PS_PD_RECON);
        return launch_pd_recon<T>(st, a);
    }

    // (1/2 of) the data fidelity at a K-map variable: fEvalX off (pdcsc.py:163-171)
    void pd_dfid(int var, double *out_dev) override {
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        const int nb = pd_recon_of(var, nullptr, true);
        const int slots[1] = {SPORCO_AMD_OUT_DFID};
        const double scales[1] = {1.0 / ((double)H * W)};
        finalize(part_a, nb, 4, 1, slots, scales, out_dev);
    }

    // irfftn(B sum_m Df_m rfftn(var)_m), (H, W, Cs, N) (pdcsc.py:184-192)
    void pd_reconstruct(int var, void *dst) override {
        (void)pd_recon_of(var, pd_rf, false);
        const int64_t csn = (int64_t)pd_Cs * N;
        inv2(pd_rf, pd_rf, pd_sreal, csn);
        SA_HIP(hipMemcpyAsync(dst, pd_sreal, sizeof(T) * (int64_t)H * W * csn, hipMemcpyDeviceToHost, st));
        sync();
    }
