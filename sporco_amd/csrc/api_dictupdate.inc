// api_dictupdate.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): PGM dictionary update, constraint projection, masked data fidelity.
    // ---- dictionary update -------------------------------------------------------------
    void ccmod_setcoef(int var) override {
        SA_REQUIRE(var_is_valid(var) && !var_is_complex(var) && !var_is_dict_sized(var),
                   "ccmod_setcoef needs an X-sized real variable");
        before_read(var);
        gramz_valid = false;
        zsf_valid = dism_valid = zfv_valid = false;
        // A multi-channel dictionary whose coefficient maps carry the channels as well (the
        // reference's broadcasting admits it, tests/admm/test_ccmod.py:278-295: Cd independent
        // single-channel updates sharing rho and the residuals), staged in the consensus blocks'
        // layout (H, W, N, Cd, K) -- VAR_CX -- and kept in a spectrum of that size
        z_chan = Cd > 1 && var == SPORCO_AMD_VAR_CX;
        SA_REQUIRE(!cplx_pair || z_chan, "complex pair mode: the coefficient maps come per channel (VAR_CX)");
        if (z_chan) {
            if (!zf_ch) SA_HIP(hipMalloc((void **)&zf_ch, sizeof(cx<T>) * EF * Cd));
            zf_tiled = false;
            fwd2(rv(var), nullptr, T(0), zf_ch, P * Cd);
            if (cplx_pair) pm_pair(zf_ch, zf_ch, CN, K, 0);
            SA_HIP(hipMemsetAsync(rv(var), 0, sizeof(T) * E * Cd, st));   // (X_n = 0 before a solve)
            return;
        }
        // (the generic consensus D-step and the single-copy ADMM D-step read Zf in the natural
        // layout)
        // (K > 64: the slab forms of the column transform and of the PGM gradient; the ADMM
        // dictionary updates read Zf in the natural layout there)
        if (rows_ok && (cols256 || mr) && (fused || (fused_slabs && !cns_active && !mr)) &&
            !(cns_active && !cns_fused()) && !eq_active) {
            // rows then columns, register-resident, straight into the tile-major layout
            // (the iterate in its single-array form: Y = prox(V) is derived inside the row pass
            // -- with s2 = 0 the kernel transforms Y - 0 U = Y -- instead of being written out first,
            // under the options the iterate was produced with)
            const bool from_v = var == SPORCO_AMD_VAR_Y && it.form == IterForm::FusedV;
            cx<T> *Zf = cv(SPORCO_AMD_VAR_ZF);
            auto ra = rows_fwd_args(Zf);
            if (from_v) {
                sporco_amd_admm_params q = last_p;
                q.flags = it.cur.flags();
                ra = rows_fwd_args(it.cur, q, Zf);
            } else {
                ra.y = rv(var);
            }
            ra.s2 = T(0);
            {
                ProfScope ps(prof, PS_SETCOEF_ROWS);
                launch_rows_fwd<T>(st, ra);
            }
            PgmColsArgs<T> ca;
            ca.yf = nullptr;
            ca.xf_old = nullptr;
            ca.t = cv(SPORCO_AMD_VAR_ZF);
            ca.yf_new = nullptr;
            ca.ey = nullptr;
            ca.dft = nullptr;
            ca.sft = nullptr;
            ca.twA = twA;
            ca.twB = twB;
            ca.inv_L = T(0);
            ca.beta = T(0);
            ca.H = H;
            ca.W = W;
            ca.CN = CN;
            ca.K = K;
            ca.want_stats = 0;
            ca.partials = nullptr;
            {
                ProfScope ps(prof, PS_SETCOEF_COLS);
                launch_cols_fft<T>(st, ca);
            }
            zf_tiled = true;
            return;
        }
        zf_tiled = false;
        fwd2(rv(var), nullptr, T(0), cv(SPORCO_AMD_VAR_ZF), P);
    }

    // Groups of images per row frequency in the tiled gradient (one workgroup per (row frequency,
    // group), the groups' partial gradients summed afterwards): enough to fill the chip.  For the
    // kernel of 16-row threads (K = 64, H <= 256: one 16-wave workgroup per CU at H = 256, two
    // 8-wave ones at H = 128) the count that minimises rounds x images per workgroup -- 129 row
    // frequencies x 6 groups are 774 workgroups, four rounds on 256 CUs for three rounds of work;
    // 5 groups: 645, three rounds of 13 images instead of four of 11.
    int ccmod_group_count() const {
        int g0 = (int)ceil_div(768, Wf);
        if (K == 64 && H <= 256) {
            const int64_t slots = (int64_t)current_device_cus() * (H == 256 ? 1 : 2);
            int64_t best = 0;
            for (int g = 1; g <= 8; ++g) {
                const int64_t cost = ceil_div((int64_t)Wf * g, slots) * ceil_div(CN, g);
                if (g == 1 || cost < best) best = cost, g0 = g;
            }
        }
        if (g0 > CN) g0 = CN;
        return g0 > 8 ? 8 : g0;
    }

    void ccmod_grad(int var, bool write_grad, double *out_dev) override {
        if (!have_signal) throw Error(SPORCO_AMD_ESTATE, "set_signal must be called first");
        SA_REQUIRE(var_is_valid(var) && var_is_complex(var) && var_is_dict_sized(var),
                   "ccmod_grad needs a dictionary-sized frequency-domain variable");
        if (zf_tiled) {
            // fixed groups of tiles per workgroup; enough groups to fill the chip
            if (!gpart) {
                ccmod_groups = ccmod_group_count();
                SA_HIP(hipMalloc((void **)&gpart, sizeof(cx<T>) * npix * K * ccmod_groups));
            }
            CcmodTiledArgs<T> ga;
            ga.zf = cv(SPORCO_AMD_VAR_ZF);
            ga.d = cv(var);
            ga.sft = sft;
            ga.gpart = write_grad ? gpart : nullptr;
            ga.H = H;
            ga.W = W;
            ga.CN = CN;
            ga.K = K;
            ga.G = ccmod_groups;
            ga.partials = part_a;
            if (K > 64) {
                // (one row of sums per tile: part_f holds 2 * slabs doubles per tile)
                if (!ccmod_r) SA_HIP(hipMalloc((void **)&ccmod_r, sizeof(cx<T>) * (int64_t)Wf * CN * H));
                ga.qpart = qpart;
                ga.rbuf = ccmod_r;
                ga.partials = part_f;
            }
            int64_t nwg;
            {
                ProfScope ps(prof, PS_CCMOD_GRAD);
                nwg = launch_ccmod_grad_tiled<T>(st, ga);
                if (write_grad)
                    launch_sum_groups<T>(st, gpart, cv(SPORCO_AMD_VAR_DGF), npix * K, ccmod_groups);
            }
            const int slots[3] = {SPORCO_AMD_PGM_F, SPORCO_AMD_PGM_DFID, SPORCO_AMD_PGM_HESS};
            const double scales[3] = {0.5, 1.0 / ((double)H * W), 1.0};
            finalize(ga.partials, (int)nwg, 4, 3, slots, scales, out_dev);
            return;
        }
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            nb = launch_ccmod_grad<T>(st, zf_nat(), cv(var), cv(SPORCO_AMD_VAR_SF),
                                      write_grad ? cv(SPORCO_AMD_VAR_DGF) : nullptr, npix, CN, K, W,
                                      part_a, Cd, z_chan);
        }
        const int slots[3] = {SPORCO_AMD_PGM_F, SPORCO_AMD_PGM_DFID, SPORCO_AMD_PGM_HESS};
        const double scales[3] = {0.5, 1.0 / ((double)H * W), 1.0};
        finalize(part_a, nb, 3, 3, slots, scales, out_dev);
    }

    void pcn_project(const T *v, T *out, int dH, int dW, bool zm, double *out_dev) {
        SA_REQUIRE(dH >= 1 && dW >= 1 && dH <= (depth > 1 ? Hs : H) && dW <= W, "filter support out of range");
        int nb;
        {
            ProfScope ps(prof, PS_OTHER);
            launch_pcn_stats<T>(st, v, pcn_stats_buf(), H, W, K, dH, dW, zm, Cd, fsz());
            nb = launch_pcn_apply<T>(st, v, pcn_stats_buf(), out, H, W, K, dH, dW, part_b, Ku, Cd, fsz());
        }
        if (out_dev) {
            const int slots[1] = {0};
            const double scales[1] = {1.0};
            finalize(part_b, nb, 1, 1, slots, scales, out_dev);
        }
    }

    void ccmod_prox_step(double L, int dH, int dW, bool zm) override {
        cx<T> *Vf = cv(SPORCO_AMD_VAR_DVF);
        {
            ProfScope ps(prof, PS_PGM);
            launch_axpy_c<T>(st, cv(SPORCO_AMD_VAR_DYF), cv(SPORCO_AMD_VAR_DGF), Vf, (T)(-1.0 / L),
                             npix * KD());
        }
        T *X = rv(SPORCO_AMD_VAR_DX);
        inv2(Vf, dwork_buf(), X, KD());
        pcn_project(X, X, dH, dW, zm, nullptr);
        fwd2(X, nullptr, T(0), cv(SPORCO_AMD_VAR_DXF), KD());
    }

    // One projected stochastic gradient step on the X-step's dictionary (onlinecdl.py:310-333):
    // G = irfftn(Df - eta * gradient), D = Pcn(G); out[CNSTR] = sum (Pcn(G) - G)^2 (:398).
    void ccmod_sgd_step(double eta, int dH, int dW, bool zm, double *out_dev) override {
        if (!have_dict) throw Error(SPORCO_AMD_ESTATE, "set_dict must be called first");
        SA_REQUIRE(dH >= 1 && dW >= 1 && dH <= H && dW <= W, "filter support out of range");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        cx<T> *Vf = cv(SPORCO_AMD_VAR_DVF);
        {
            ProfScope ps(prof, PS_PGM);
            launch_axpy_c<T>(st, cv(SPORCO_AMD_VAR_DF), cv(SPORCO_AMD_VAR_DGF), Vf, (T)(-eta),
                             npix * KD());
        }
        T *X = rv(SPORCO_AMD_VAR_DX);
        inv2(Vf, dwork_buf(), X, KD());
        int nb;
        {
            ProfScope ps(prof, PS_OTHER);
            launch_pcn_stats<T>(st, X, pcn_stats_buf(), H, W, K, dH, dW, zm, Cd, fsz());
            nb = launch_pcn_apply<T>(st, X, pcn_stats_buf(), X, H, W, K, dH, dW, part_b, Ku, Cd, fsz());
        }
        const int slots[1] = {SPORCO_AMD_OUT_CNSTR};
        const double scales[1] = {1.0};
        finalize(part_b, nb, 1, 1, slots, scales, out_dev);
        fwd2(X, nullptr, T(0), cv(SPORCO_AMD_VAR_DXF), KD());
    }

    void ccmod_cnstr(int dH, int dW, bool zm, double *out_dev) override {
        pcn_project(rv(SPORCO_AMD_VAR_DX), nullptr, dH, dW, zm, out_dev);
    }

    void ccmod_getdict(int dH, int dW, void *dst) override {
        SA_REQUIRE(dH >= 1 && dW >= 1 && dH <= H && dW <= W, "filter support out of range");
        std::vector<T> tmp;
        void *out = dst;
        if (K != Ku) {
            tmp.resize((size_t)dH * dW * K);
            out = tmp.data();
        }
        // (rows of dW pixels x Cd channels x K filters; Cd > 1 is never padded)
        SA_HIP(hipMemcpy2DAsync(out, sizeof(T) * (size_t)dW * KD(), rv(SPORCO_AMD_VAR_DX),
                                sizeof(T) * (size_t)W * KD(), sizeof(T) * (size_t)dW * KD(),
                                (size_t)dH, hipMemcpyDeviceToHost, st));
        sync();
        if (K != Ku) {   // drop the padding filter
            T *o = static_cast<T *>(dst);
            for (int64_t r = 0; r < (int64_t)dH * dW; ++r)
                for (int k = 0; k < Ku; ++k) o[r * Ku + k] = tmp[(size_t)(r * K + k)];
        }
    }

    void setdict_from_dstep(int dH, int dW) override {
        before_dict_change();
        SA_HIP(hipMemcpyAsync(cv(SPORCO_AMD_VAR_DF), cv(SPORCO_AMD_VAR_DXF),
                              sizeof(cx<T>) * npix * KD(), hipMemcpyDeviceToDevice, st));
        ism_valid = false;
        if (Cd == 1) {
            ProfScope ps(prof, PS_OTHER);
            launch_gram<T>(st, cv(SPORCO_AMD_VAR_DF), gram, npix, K);
        }
        refresh_fused_dict();
        dH_ = dH;
        dW_ = dW;
        have_dict = true;
    }

    // ---- masked data fidelity (pgm ConvBPDNMask / ConvCnstrMODMask) -------------------------
    // Gradient of (1/2) ||W (sum_m d_m * x_m - s)||^2 with respect to the coefficient spectra
    // (dstep false: `var` is X-sized, result in VAR_GF; pgm/cbpdn.py:454-477) or to the
    // dictionary (dstep true: `var` is dictionary sized, result in VAR_DGF; pgm/ccmod.py:552-575):
    // residual -> irfftn -> W^2 -> rfftn -> adjoint.  With write_grad false the residual is
    // weighted by W only and nothing is written back: out[PGM_DFID] = sum (W R)^2 (twice the
    // data fidelity term, :481-489) and out[PGM_F] = (1/2) sum_half |rfftn(W R)|^2 (the
    // unnormalised DFT-domain value backtracking compares, :493-506).
    // (mode 0: evaluation, 1: gradient with W^2, 2: gradient with the residual weighted by W
    // once -- the form of the online learner's dictionary step, onlinecdl.py:578-580)
    void masked_grad(int var, bool dstep, int mode, double *out_dev) override {
        const bool write_grad = mode != 0;
        // (multi-channel dictionary, Cd = Cs > 1: the coefficient maps have no channel axis, the
        // residual has the signal's -- inner products and adjoints over (channel, filter))
        if (!have_signal) throw Error(SPORCO_AMD_ESTATE, "set_signal must be called first");
        SA_REQUIRE(var_is_valid(var) && var_is_complex(var) && var_is_dict_sized(var) == dstep &&
                       var != SPORCO_AMD_VAR_SF && var != SPORCO_AMD_VAR_DF,
                   "masked_grad: variable of the wrong kind");
        before_read(var);
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        cx<T> *Sf = cv(SPORCO_AMD_VAR_SF);
        {   // residual spectrum R = sum_m Df Xf - Sf, signal sized (npix, C N)
            ProfScope ps(prof, PS_PGM);
            if (dstep) {
                need_natural(SPORCO_AMD_VAR_ZF);
                if (Cd > 1) launch_mc_inner<T>(st, cv(var), zf_nat(), innerb, npix, Cd, N, K, z_chan);
                else launch_inner<T>(st, cv(var), cv(SPORCO_AMD_VAR_ZF), innerb, npix, CN, K);
            } else {
                require_ready();
                if (Cd > 1) launch_mc_inner<T>(st, cv(SPORCO_AMD_VAR_DF), cv(var), innerb, npix, Cd, N, K);
                else launch_inner<T>(st, cv(SPORCO_AMD_VAR_DF), cv(var), innerb, npix, CN, K);
            }
            launch_lincomb<T>(st, innerb, T(1), innerb, T(-1), Sf, T(0), nullptr, npix * CNs);
        }
        inv2(innerb, innerb, sreal, CNs);
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            nb = launch_mask_apply<T>(st, sreal, have_wdat ? wdat : Weight<T>(), mode == 1, H, W, Cs, N,
                                      part_a);
        }
        {
            const int slots[1] = {SPORCO_AMD_PGM_DFID};
            const double scales[1] = {1.0};
            finalize(part_a, nb, 1, 1, slots, scales, out_dev);
        }
        fwd2(sreal, nullptr, T(0), innerb, CNs);
        if (!write_grad) {
            {
                ProfScope ps(prof, PS_PGM);
                nb = launch_pair_stats<T>(st, innerb, nullptr, nullptr, npix, CNs, W, part_b);
            }
            const int slots[1] = {SPORCO_AMD_PGM_F};
            const double scales[1] = {0.5};
            finalize(part_b + 2, nb, 4, 1, slots, scales, out_dev);
            return;
        }
        ProfScope ps(prof, PS_PGM);
        if (dstep) {
            if (Cd > 1)
                launch_mc_zf_adjoint<T>(st, zf_nat(), innerb, cv(SPORCO_AMD_VAR_DGF), npix, Cd, N, K, z_chan);
            else
                launch_zf_adjoint<T>(st, cv(SPORCO_AMD_VAR_ZF), innerb, cv(SPORCO_AMD_VAR_DGF), npix, CN, K);
        } else if (Cd > 1) {
            launch_mc_conj_outer<T>(st, cv(SPORCO_AMD_VAR_DF), innerb, cv(SPORCO_AMD_VAR_GF), npix, Cd, N, K,
                                    false);
        } else {
            launch_conj_outer<T>(st, cv(SPORCO_AMD_VAR_DF), innerb, cv(SPORCO_AMD_VAR_GF), npix, CN, K);
        }
    }
