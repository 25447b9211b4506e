// api_consensus.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ADMM consensus dictionary updates (plain and mask-decoupled).
    // ---- ADMM consensus dictionary update -------------------------------------------------
    // Multi-channel dictionary (Cd > 1; admm/ccmod.py:696-698, :766-822): one dictionary copy
    // (H, W, Cd, K) per image -- blocks laid out (H, W, N, Cd, K), so that every kernel below
    // sees N blocks of KD() = Cd K "filters" -- whose Cd channels share the image's matrix in
    // the per-image solve (launch_sm_solve per_grp = Cd, the signal spectrum transposed to
    // (npix, N, Cd) to follow the systems).  Generic chain only.
    void cns_init(const void *Y0, double rho) override {
        SA_REQUIRE(rho != 0.0, "rho must be nonzero");
        cns_active = true;
        T *Y = rv(SPORCO_AMD_VAR_DX), *U = rv(SPORCO_AMD_VAR_CU);
        (void)rv(SPORCO_AMD_VAR_CX);
        SA_HIP(hipMemsetAsync(U, 0, sizeof(T) * E * Cd, st));
        if (Y0) {
            host_copy(SPORCO_AMD_VAR_DX, const_cast<void *>(Y0), true);
            // U_n = Y0 / rho for every image: 0 - (-1/rho) * Y through the Y - s U kernel
            ProfScope ps(prof, PS_OTHER);
            launch_cns_yu<T>(st, Y, U, U, T(0), (int64_t)H * W, CN, (int)KD());
            launch_scale<T>(st, U, (T)(1.0 / rho), E * Cd);
        } else {
            SA_HIP(hipMemsetAsync(Y, 0, var_bytes(SPORCO_AMD_VAR_DX), st));
        }
        fwd2(Y, nullptr, T(0), cv(SPORCO_AMD_VAR_DXF), KD());
        if (cplx_pair) pm_pair(cv(SPORCO_AMD_VAR_DXF), cv(SPORCO_AMD_VAR_DXF), 1, K, 1);
        sync();
    }

    cx<T> *cns_w = nullptr, *cns_sft = nullptr;   // Cd > 1: column-pass scratch, transposed Sf
    cx<T> *zf_ch = nullptr;     // Cd > 1, channel-ful coefficient maps: spectrum (npix, N, Cd, K)
    bool z_chan = false;
    const cx<T> *zf_nat() { return z_chan ? zf_ch : cv(SPORCO_AMD_VAR_ZF); }
    // multi-scale dictionary: per-filter support sizes of the constraint projection (K ints
    // each; null: the one support the calls name)
    int *flt_h = nullptr, *flt_w = nullptr;
    int vol_dD = 1;      // volume handle: depth of the filter support (SPORCO_AMD_VOLUME_FILTER_DEPTH)
    FilterSizes fsz() const {
        FilterSizes f;
        f.h = flt_h;
        f.w = flt_w;
        if (depth > 1) {
            f.Hs = Hs;
            f.dD = vol_dD;
        }
        return f;
    }
    void set_filter_sizes(const int32_t *fh, const int32_t *fw) override {
        sync();
        if (flt_h) {
            SA_HIP(hipFree(flt_h));
            SA_HIP(hipFree(flt_w));
            flt_h = flt_w = nullptr;
        }
        if (!fh || !fw) return;
        std::vector<int> h((size_t)K, 0), w((size_t)K, 0);     // (padding filters: empty support)
        for (int k = 0; k < Ku; ++k) {
            SA_REQUIRE(fh[k] >= 1 && fh[k] <= H && fw[k] >= 1 && fw[k] <= W, "filter size out of range");
            h[k] = fh[k];
            w[k] = fw[k];
        }
        SA_HIP(hipMalloc((void **)&flt_h, sizeof(int) * K));
        SA_HIP(hipMalloc((void **)&flt_w, sizeof(int) * K));
        SA_HIP(hipMemcpy(flt_h, h.data(), sizeof(int) * K, hipMemcpyHostToDevice));
        SA_HIP(hipMemcpy(flt_w, w.data(), sizeof(int) * K, hipMemcpyHostToDevice));
    }
    void cns_buffers() {
        if (cns_f) return;
        const int64_t npixr = (int64_t)H * W;
        SA_HIP(hipMalloc((void **)&cns_f, sizeof(cx<T>) * EF * Cd));
        SA_HIP(hipMalloc((void **)&cns_m, sizeof(T) * npixr * KD()));
        SA_HIP(hipMalloc((void **)&cns_yold, sizeof(T) * npixr * KD()));
        if (Cd > 1) {
            SA_HIP(hipMalloc((void **)&cns_w, sizeof(cx<T>) * EF * Cd));
            SA_HIP(hipMalloc((void **)&cns_sft, sizeof(cx<T>) * npix * CNs));
        }
    }
    void *cns_mean_ptr(int64_t *count) override {
        cns_buffers();
        *count = (int64_t)H * W * KD();
        return cns_m;
    }

    // ---- consensus update with mask decoupling (ConvCnstrMODMaskDcpl_Consensus) ----------------
    void cns_md_init(const void *S) override {
        SA_REQUIRE(S != nullptr, "S is null");
        const size_t nb = sizeof(T) * (int64_t)H * W * CNs;
        if (!md_s) SA_HIP(hipMalloc((void **)&md_s, nb));
        SA_HIP(hipMemcpyAsync(md_s, S, nb, hipMemcpyHostToDevice, st));
        SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_DMY0), 0, nb, st));
        SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_DMU0), 0, nb, st));
        sync();
    }

    // One iteration of sporco/admm/ccmodmd.py:766-1083 in the order of ADMM.solve
    // (admm.py:331-367): xstep (:922-939, the consensus solve with rho = 1 and S + Y1 - U1 in
    // the signal's place), relax_AX (:899-918), ystep (:943-952), ustep (:956-963), and the
    // sums of compute_residuals (:976-1034) / obfn_dfd (:966-972).  Generic FFT chain.
    // Multi-channel dictionary (Cd > 1; the reference's examples/scripts/cdl/cbpdndl_md_clr.py):
    // one (Cd, K) block per image as in cns_iter -- systems and block spectra in (image, channel)
    // order, the signal-sized block (Y1, U1, S, the mask) in the signal's (channel, image) order,
    // its spectra transposed on the way in and out of the block arithmetic.
    void cns_md_iter(const sporco_amd_cns_params &p, double *out_dev) {
        SA_REQUIRE(md_s != nullptr, "cns_md_init must be called first");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        need_natural(SPORCO_AMD_VAR_ZF);
        const int64_t npixr = (int64_t)H * W, ns = npixr * CNs;
        const int KDi = (int)KD();
        const int64_t PD = P * Cd;
        const int64_t nblk = npix * CN * Cd;        // (frequency, image, channel) rows
        const T us = (T)p.u_scale;
        T *Y = rv(SPORCO_AMD_VAR_DX), *X = rv(SPORCO_AMD_VAR_CX), *U = rv(SPORCO_AMD_VAR_CU);
        T *Y1 = rv(SPORCO_AMD_VAR_DMY0), *U1 = rv(SPORCO_AMD_VAR_DMU0);
        const cx<T> *Zf = zf_nat();
        cns_buffers();
        cx<T> *wk = Cd > 1 ? cns_w : work_buf();
        // (signal-sized spectra in the blocks' order: the transposed copy when Cd > 1)
        auto to_blocks = [&](cx<T> *sig) -> cx<T> * {
            if (Cd == 1) return sig;
            ProfScope ps(prof, PS_OTHER);
            launch_swap_inner<T>(st, sig, cns_sft, npix, Cd, N);
            return cns_sft;
        };
        if (p.phase != 2) {
        // xstep: ZSf = conj(Zf) rfftn(S + Y1 - U1); X_n = irfftn(SM(Zf_n, 1, ZSf_n + rfftn(Y - U_n)))
        {
            ProfScope ps(prof, PS_OTHER);
            // (U1 takes no part in update_rho's `U /= rsf`, admm.py:573: the reference rescales
            // the consensus duals only, so the pending scale does not apply to it)
            launch_md_pre<T>(st, Y1, U1, md_s, sreal, T(1), ns);
        }
        fwd2(sreal, nullptr, T(0), innerb, CNs);
        const cx<T> *sfb = to_blocks(innerb);
        {
            ProfScope ps(prof, PS_FFT_R2C);
            fft_r2c<T>(st, planW, Y, U, us, cns_f, H, PD, (int64_t)W * PD, PD, (int64_t)Wf * PD, PD, 0,
                       0, KDi);
        }
        {
            ProfScope ps(prof, PS_FFT_C2C_FWD);
            fft_c2c<T>(st, planH, false, cns_f, cns_f, 1, (int64_t)Wf * PD, 0, (int64_t)Wf * PD, 0,
                       (int64_t)Wf * PD, T(1));
        }
        // LinSolveCheck (ccmod.py:783-792, as in cns_iter; the XRRS slots carry block-1 sums in
        // this call, so the three sums go to the L1, RGR and CGN slots)
        const bool lsc = p.flags & F_XRRS;
        if (lsc) {
            ProfScope ps(prof, PS_OTHER);
            launch_cns_xrrs_rhs<T>(st, Zf, sfb, cns_f, T(1), dwork_buf(), npix, CN * Cd, K, Cd, z_chan);
        }
        {
            ProfScope ps(prof, PS_SM_SOLVE);
            launch_sm_solve<T>(st, cns_f, cns_f, Zf, sfb, nullptr, T(1), npix, CN * Cd, K, W, false,
                               false, part_a, nullptr, z_chan ? 1 : Cd);
        }
        if (lsc) {
            int nbx;
            {
                ProfScope ps(prof, PS_OTHER);
                nbx = launch_cns_xrrs_fin<T>(st, Zf, cns_f, T(1), dwork_buf(), npix, CN * Cd, K, part_a, Cd,
                                             z_chan);
            }
            const int xslots[3] = {SPORCO_AMD_OUT_L1, SPORCO_AMD_OUT_RGR, SPORCO_AMD_OUT_CGN};
            const double xscales[3] = {1.0, 1.0, 1.0};
            finalize(part_a, nbx, 3, 3, xslots, xscales, out_dev);
        }
        // relax_AX, block 1: AX1nr_n = irfftn(sum_m Zf_{n,m} Xf_{n,m}) -- the inner product of
        // every (frequency, image) row with itself-indexed coefficients: npix * CN "pixels"
        // (the Cd channel blocks of an image against the image's row when they share it)
        {
            ProfScope ps(prof, PS_OTHER);
            if (Cd == 1) {
                launch_inner<T>(st, Zf, cns_f, innerb, npix * CN, 1, K);
            } else {
                if (z_chan) launch_inner<T>(st, Zf, cns_f, cns_sft, nblk, 1, K);
                else launch_inner<T>(st, Zf, cns_f, cns_sft, npix * CN, Cd, K);
                launch_swap_inner<T>(st, cns_sft, innerb, npix, N, Cd);
            }
        }
        inv2(cns_f, wk, X, PD);
        inv2(innerb, innerb, sreal, CNs);
        // consensus part: Y = Pcn(mean_n(alpha X_n + (1 - alpha) Y + U_n))
        SA_HIP(hipMemcpyAsync(cns_yold, Y, sizeof(T) * npixr * KDi, hipMemcpyDeviceToDevice, st));
        {
            ProfScope ps(prof, PS_OTHER);
            launch_cns_mean<T>(st, X, U, cns_yold, cns_m, (T)p.rlx, us, npixr, CN, KDi);
        }
        }   // phase != 2
        if (p.phase == 1) return;
        pcn_project(cns_m, Y, p.dH, p.dW, p.zero_mean != 0, nullptr);
        // block 1: AX1 = alpha AX1nr + (1 - alpha)(Y1 + S); Y1 = rho (AX1 + U1 - S) / (W^2 + rho);
        // U1 += AX1 - Y1 - S  -- the block-0 step of ConvBPDNMaskDcpl, same kernel
        MdY0Args<T> ya;
        ya.ax0nr = sreal;
        ya.y0 = Y1;
        ya.u0 = U1;
        ya.s = md_s;
        ya.w = have_wdat ? wdat : Weight<T>();
        ya.rho = (T)p.rho;
        ya.rlx = (T)p.rlx;
        ya.us = T(1);
        ya.geval_y = 1;
        ya.H = H;
        ya.W = W;
        ya.C = Cs;
        ya.N = N;
        int nb;
        {
            ProfScope ps(prof, PS_OTHER);
            nb = launch_md_y0step<T>(st, ya, part_a);
        }
        {
            const int slots[4] = {SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2,
                                  SPORCO_AMD_OUT_XRRS_B2, SPORCO_AMD_OUT_CGIT};
            const double scales[4] = {1, 1, 1, 1};
            finalize(part_a, nb, 5, 4, slots, scales, out_dev);
        }
        // consensus ustep + the X-sized sums
        {
            ProfScope ps(prof, PS_ADMM_POST);
            nb = launch_cns_ustep<T>(st, X, U, cns_yold, Y, (T)p.rlx, us, npixr, CN, KDi, part_b);
        }
        {
            const int slots[3] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_U2};
            const double scales[3] = {1, 1, 1};
            finalize(part_b, nb, 4, 3, slots, scales, out_dev);
        }
        {
            ProfScope ps(prof, PS_OTHER);
            nb = launch_cns_ystats<T>(st, cns_yold, Y, npixr * KDi, part_a);
        }
        {
            const int slots[2] = {SPORCO_AMD_OUT_L21, SPORCO_AMD_OUT_Y2};   // (|Y - Yprev|^2 unused)
            const double scales[2] = {0, 1};
            finalize(part_a, nb, 2, 2, slots, scales, out_dev);
        }
        fwd2(Y, nullptr, T(0), cv(SPORCO_AMD_VAR_DXF), KDi);
        if (p.flags & F_RESID) {
            // dual residual: A^T u = U_n + irfftn(conj(Zf_n) rfftn(U1_n)), new duals (:993-996)
            fwd2(U1, nullptr, T(0), innerb, CNs);
            fwd2(U, nullptr, T(0), cns_f, PD);
            const cx<T> *u1b = to_blocks(innerb);
            {
                ProfScope ps(prof, PS_OTHER);
                if (Cd == 1 || z_chan) launch_conj_outer<T>(st, Zf, u1b, wk, nblk, 1, K);
                else launch_conj_outer<T>(st, Zf, u1b, wk, npix * CN, Cd, K);
                launch_lincomb<T>(st, wk, T(1), wk, T(1), cns_f, T(0), nullptr, EF * Cd);
                nb = launch_pair_stats<T>(st, wk, nullptr, nullptr, npix, PD, W, part_b);
            }
            const int slots[1] = {SPORCO_AMD_OUT_S2};
            const double scales[1] = {1.0 / ((double)H * W)};
            finalize(part_b, nb, 4, 1, slots, scales, out_dev);
        }
        if (p.flags & F_OBJ) {
            // (1/2) |W irfftn(sum_m Zf Yf - Sf)|^2 at the consensus variable (:961-970)
            {
                ProfScope ps(prof, PS_OTHER);
                if (Cd == 1) launch_inner<T>(st, cv(SPORCO_AMD_VAR_DXF), Zf, innerb, npix, CN, K);
                else launch_mc_inner<T>(st, cv(SPORCO_AMD_VAR_DXF), Zf, innerb, npix, Cd, N, K, z_chan);
                launch_lincomb<T>(st, innerb, T(1), innerb, T(-1), cv(SPORCO_AMD_VAR_SF), T(0),
                                  nullptr, npix * CNs);
            }
            inv2(innerb, innerb, sreal, CNs);
            {
                ProfScope ps(prof, PS_OTHER);
                nb = launch_mask_apply<T>(st, sreal, have_wdat ? wdat : Weight<T>(), false, H, W, Cs, N,
                                          part_a);
            }
            const int slots[1] = {SPORCO_AMD_OUT_DFID};
            const double scales[1] = {1.0};
            finalize(part_a, nb, 1, 1, slots, scales, out_dev);
            int nbc;
            {
                ProfScope ps(prof, PS_OTHER);
                launch_pcn_stats<T>(st, Y, pcn_stats_buf(), H, W, K, p.dH, p.dW, p.zero_mean != 0, Cd, fsz());
                nbc = launch_pcn_apply<T>(st, Y, pcn_stats_buf(), nullptr, H, W, K, p.dH, p.dW, part_b,
                                          Ku, Cd, fsz());
            }
            const int cslots[1] = {SPORCO_AMD_OUT_CNSTR};
            const double cscales[1] = {1.0};
            finalize(part_b, nbc, 1, 1, cslots, cscales, out_dev);
        }
    }

    void cns_iter(const sporco_amd_cns_params &p, double *out_dev) override {
        if (!have_signal) throw Error(SPORCO_AMD_ESTATE, "set_signal must be called first");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        SA_REQUIRE(p.phase >= 0 && p.phase <= 2, "phase must be 0, 1 or 2");
        if (p.mask_dcpl) {
            SA_REQUIRE(depth == 1, "volume handle: no mask decoupling");
            cns_md_iter(p, out_dev);
            return;
        }
        // LinSolveCheck (F_XRRS; a diagnostic): the generic chain, whose solve sees the
        // right-hand sides in the natural layout
        const bool lsc = p.flags & F_XRRS;
        const bool fusedx = cns_fused() && !lsc && Cd == 1;
        const int KDi = (int)KD();              // "filters" of a consensus block: Cd K
        const int64_t PD = P * Cd;              // columns of the blocks' spectra: N Cd K
        // objective at the consensus variable Y (FLAG_FEVAL_Y / FLAG_GEVAL_Y: AuxVarObj, the
        // class default) or at the blocks X_n (fEvalX: admm/ccmod.py:870-889) and their mean
        // (gEvalY False: admm/admm.py:1641-1646)
        const bool dfid_x = (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y);
        const bool cns_x = (p.flags & F_OBJ) && !(p.flags & F_GEVAL_Y);
        SA_REQUIRE(!(cns_x && p.phase != 0), "the constraint measure at mean(X) needs all the images");
        SA_REQUIRE(!cplx_pair || (z_chan && !dfid_x && !cns_x && p.phase == 0),
                   "complex pair mode: per-channel coefficient maps, objective at Y, no image shards");
        if (fusedx) {
            if (!zf_tiled) relayout(SPORCO_AMD_VAR_ZF, true), zf_tiled = true;
        } else {
            need_natural(SPORCO_AMD_VAR_ZF);
        }
        const int64_t npixr = (int64_t)H * W;
        T *Y = rv(SPORCO_AMD_VAR_DX), *X = rv(SPORCO_AMD_VAR_CX), *U = rv(SPORCO_AMD_VAR_CU);
        const cx<T> *Zf = zf_nat();
        cns_buffers();
        if (p.phase != 2) {
        // xstep (ccmod.py:766-778): X_n = irfftn(SM(Zf_n, rho, conj(Zf_n) Sf_n + rho rfftn(Y - U_n)));
        // Y is broadcast over the images by the row transform itself
        if (fusedx) {
            // the three register-resident kernels of the sparse coding step, with the
            // coefficient spectra of each (frequency, image) tile in the dictionary's place
            if (!gramz_t) SA_HIP(hipMalloc((void **)&gramz_t, sizeof(T) * npix * CN));
            if (!gramz_valid) {
                ProfScope ps(prof, PS_OTHER);
                launch_gram_rows<T>(st, Zf, gramz_t, npix * CN, K);
                gramz_valid = true;
            }
            auto ra = rows_fwd_args(cns_f);
            ra.y = Y;
            ra.u = U;
            ra.s2 = (T)p.u_scale;
            ra.y_bcast = 1;
            run_rows_fwd(ra);
            // (the coefficient spectra of each tile in the dictionary's place, their gram per tile)
            auto fa = fused_cols_args(p.rho, false, cns_f);
            fa.dft = Zf;
            fa.gramt = gramz_t;
            fa.per_tile = 1;
            int64_t ntl;
            {
                ProfScope ps(prof, PS_FUSED_COLS);
                ntl = launch_fused_cols<T>(st, fa);
            }
            if (dfid_x) {     // (the column kernel's by-product: sum_n |Zf_n . Xf_n - Sf_n|^2)
                const int slots[1] = {SPORCO_AMD_OUT_DFID};
                const double scales[1] = {1.0 / ((double)H * W)};
                finalize(part_f, (int)ntl, 1, 1, slots, scales, out_dev);
            }
            rows_inverse_to(X, cns_f);
        } else {
        {
            ProfScope ps(prof, PS_FFT_R2C);
            fft_r2c<T>(st, planW, Y, U, (T)p.u_scale, cns_f, H, PD, (int64_t)W * PD, PD,
                       (int64_t)Wf * PD, PD, 0, 0, KDi);
        }
        {
            ProfScope ps(prof, PS_FFT_C2C_FWD);
            c2c_first_axis(false, cns_f, cns_f, PD);
        }
        if (cplx_pair) pm_pair(cns_f, cns_f, CN, K, 1);
        // the right-hand sides' signal term follows the systems: (npix, N) -- or (npix, N, Cd)
        const cx<T> *sfs = cv(SPORCO_AMD_VAR_SF);
        if (Cd > 1) {
            ProfScope ps(prof, PS_OTHER);
            launch_swap_inner<T>(st, cv(SPORCO_AMD_VAR_SF), cns_sft, npix, Cd, N);
            sfs = cns_sft;
        }
        if (lsc) {
            ProfScope ps(prof, PS_OTHER);
            launch_cns_xrrs_rhs<T>(st, Zf, sfs, cns_f, (T)p.rho, dwork_buf(), npix, CN * Cd, K, Cd, z_chan);
        }
        int nbs;
        {   // (the per-image gram sum_k |Zf|^2 is formed inside the kernel)
            ProfScope ps(prof, PS_SM_SOLVE);
            nbs = launch_sm_solve<T>(st, cns_f, cns_f, Zf, sfs, nullptr, (T)p.rho, npix, CN * Cd, K, W,
                                     dfid_x, false, part_a, nullptr, z_chan ? 1 : Cd);
        }
        if (dfid_x) {
            const int slots[1] = {SPORCO_AMD_OUT_DFID};
            const double scales[1] = {1.0 / ((double)H * W)};
            finalize(part_a, nbs, 4, 1, slots, scales, out_dev);
        }
        if (lsc) {
            int nbx;
            {
                ProfScope ps(prof, PS_OTHER);
                nbx = launch_cns_xrrs_fin<T>(st, Zf, cns_f, (T)p.rho, dwork_buf(), npix, CN * Cd, K, part_a,
                                             Cd, z_chan);
            }
            const int xslots[3] = {SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2, SPORCO_AMD_OUT_XRRS_B2};
            const double xscales[3] = {1.0, 1.0, 1.0};
            finalize(part_a, nbx, 3, 3, xslots, xscales, out_dev);
        }
        if (cplx_pair) pm_pair(cns_f, cns_f, CN, K, 2);
        inv2(cns_f, Cd > 1 ? cns_w : work_buf(), X, PD);
        }
        // relax + ystep: Y = Pcn(mean_n(alpha X_n + (1 - alpha) Y + U_n))
        SA_HIP(hipMemcpyAsync(cns_yold, Y, sizeof(T) * npixr * KDi, hipMemcpyDeviceToDevice, st));
        {
            ProfScope ps(prof, PS_OTHER);
            launch_cns_mean<T>(st, X, U, cns_yold, cns_m, (T)p.rlx, (T)p.u_scale, npixr, CN, KDi);
        }
        }   // phase != 2
        if (p.phase == 1) return;
        pcn_project(cns_m, Y, p.dH, p.dW, p.zero_mean != 0, nullptr);
        // ustep + the X-sized sums
        int nb;
        {
            ProfScope ps(prof, PS_ADMM_POST);
            nb = launch_cns_ustep<T>(st, X, U, cns_yold, Y, (T)p.rlx, (T)p.u_scale, npixr, CN, KDi,
                                     part_b);
        }
        {
            const int slots[3] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_U2};
            const double scales[3] = {1, 1, 1};
            finalize(part_b, nb, 4, 3, slots, scales, out_dev);
        }
        {
            ProfScope ps(prof, PS_OTHER);
            nb = launch_cns_ystats<T>(st, cns_yold, Y, npixr * KDi, part_a);
        }
        {
            const int slots[2] = {SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_Y2};
            const double scales[2] = {1, 1};
            finalize(part_a, nb, 2, 2, slots, scales, out_dev);
        }
        // the consensus dictionary's spectrum (for the objective, getdict / setdict_from_dstep)
        fwd2(Y, nullptr, T(0), cv(SPORCO_AMD_VAR_DXF), KDi);
        if (cplx_pair) pm_pair(cv(SPORCO_AMD_VAR_DXF), cv(SPORCO_AMD_VAR_DXF), 1, K, 1);
        if (p.flags & F_OBJ) {
            const int slots[1] = {SPORCO_AMD_OUT_DFID};
            const double scales[1] = {1.0 / ((double)H * W)};
            if (dfid_x) {
                // (already summed by the X-step)
            } else if (zf_tiled) {
                if (!gpart) {
                    ccmod_groups = ccmod_group_count();
                    SA_HIP(hipMalloc((void **)&gpart, sizeof(cx<T>) * npix * K * ccmod_groups));
                }
                CcmodTiledArgs<T> ga;
                ga.zf = Zf;
                ga.d = cv(SPORCO_AMD_VAR_DXF);
                ga.sft = sft;
                ga.gpart = nullptr;
                ga.H = H;
                ga.W = W;
                ga.CN = CN;
                ga.K = K;
                ga.G = ccmod_groups;
                ga.partials = part_a;
                int64_t nwg;
                {
                    ProfScope ps(prof, PS_PGM);
                    nwg = launch_ccmod_grad_tiled<T>(st, ga);
                }
                finalize(part_a + 1, (int)nwg, 4, 1, slots, scales, out_dev);
            } else {
                {
                    ProfScope ps(prof, PS_OTHER);
                    nb = launch_ccmod_grad<T>(st, Zf, cv(SPORCO_AMD_VAR_DXF), cv(SPORCO_AMD_VAR_SF),
                                              nullptr, npix, CN, K, W, part_a, Cd, z_chan);
                }
                // (column 0 in the complex pair mode: see dstep_iter)
                finalize(part_a + (cplx_pair ? 0 : 1), nb, 3, 1, slots, scales, out_dev);
            }
            int nbc;
            const T *gv = Y;
            if (cns_x) {      // g is evaluated at mean_n(X_n)
                ProfScope ps(prof, PS_OTHER);
                launch_cns_mean<T>(st, X, U, cns_yold, cns_m, T(1), T(0), npixr, CN, KDi);
                gv = cns_m;
            }
            {
                ProfScope ps(prof, PS_OTHER);
                launch_pcn_stats<T>(st, gv, pcn_stats_buf(), H, W, K, p.dH, p.dW, p.zero_mean != 0, Cd, fsz());
                nbc = launch_pcn_apply<T>(st, gv, pcn_stats_buf(), nullptr, H, W, K, p.dH, p.dW, part_b,
                                          Ku, Cd, fsz());
            }
            const int cslots[1] = {SPORCO_AMD_OUT_CNSTR};
            const double cscales[1] = {1.0};
            finalize(part_b, nbc, 1, 1, cslots, cscales, out_dev);
        }
    }
