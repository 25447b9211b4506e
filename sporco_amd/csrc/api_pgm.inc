// api_pgm.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): PGM (FISTA) sparse coding.
    // ---- PGM -----------------------------------------------------------------------
    // rows pass of the fused iteration: X = prox(irfft_W(t_in)), t_out = rfft_W(X)
    void pgm_rows_prox(const sporco_amd_pgm_params &p, const cx<T> *t_in, cx<T> *t_out, T *x,
                       double *out_dev) {
        auto ra = rows_prox_args();
        ra.t_in = t_in;
        ra.t_out = t_out;
        ra.x = x;
        ra.thr = (T)(p.lmbda / p.L);
        ra.flags = p.flags;
        ra.dH = p.dH;
        ra.dW = p.dW;
        ra.wl1 = wl1;
        int64_t nt;
        {
            ProfScope ps(prof, PS_PGM_ROWS_PROX);
            nt = launch_rows_inv_prox_fwd<T>(st, ra);
        }
        if (out_dev) {
            const int slots[1] = {SPORCO_AMD_PGM_L1};
            const double scales[1] = {1.0};
            finalize(part_rows, (int)nt, 1, 1, slots, scales, out_dev);
        }
    }

    // The residual of the masked classes on the tile-major iterates: e = sum_k Df v - Sf per
    // frequency (signal sized, one read pass over v: tiled_resid) taken to the spatial domain --
    // `pgm_rx[slot]` keeps it there, unmasked.
    T *pgm_rx[2] = {nullptr, nullptr};
    int pgm_rx_cur = 0, pgm_rx_count = 0;    // residuals at the last / last two committed Xf
    void pgm_resid_spatial(const cx<T> *v_tiled, T *r_out) {
        const int64_t ntile = (int64_t)Wf * CN;
        {
            ProfScope ps(prof, PS_PGM);
            launch_tiled_resid<T>(st, v_tiled, dft, sft, pgm_ey, ntile, H, K, Ks, CN);
            launch_permute_ab<cx<T>>(st, pgm_ey, innerb, ntile, H, 1);     // -> (H, Wf CN)
        }
        inv2(innerb, innerb, r_out, CNs);
    }
    // sreal (a spatial residual R) weighted by W^2, transformed, tile-major into e_out: the
    // residual the gradient kernel takes from memory (pgm/cbpdn.py:454-477)
    void pgm_masked_to_spectrum(cx<T> *e_out) {
        const int64_t ntile = (int64_t)Wf * CN;
        {
            ProfScope ps(prof, PS_PGM);
            (void)launch_mask_apply<T>(st, sreal, have_wdat ? wdat : Weight<T>(), true, H, W, Cs, N, part_a);
        }
        fwd2(sreal, nullptr, T(0), innerb, CNs);
        ProfScope ps(prof, PS_PGM);
        launch_permute_ab<cx<T>>(st, innerb, e_out, H, ntile, 1);          // -> (Wf CN, H)
    }

    void pgm_iter(const sporco_amd_pgm_params &p, double *out_dev) override {
        require_single_channel_dict();
        require_ready();
        if (!pgm_fused_ok())
            throw Error(SPORCO_AMD_EINVAL, "pgm_iter: shape not served by the fused kernels");
        const bool dmask = p.flags & F_DMASK;
        if (dmask)
            SA_REQUIRE(K <= 64 && !p.hold, "the masked iteration: K <= 64, no held (backtracking) trial");
        t_ready = false;
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        const int NHp = (K + 63) / 64;      // 64-filter slabs of the column kernels (1: K <= 64)
        if (!part_pgm) {
            SA_HIP(hipMalloc((void **)&part_pgm,
                             sizeof(double) * kPgmPartialStride * (int64_t)Wf * CN * NHp));
            if (NHp > 1) SA_HIP(hipMalloc((void **)&part_pgm2, sizeof(double) * 3 * (int64_t)Wf * CN));
        }
        if ((p.hold || dmask) && !pgm_ey)
            SA_HIP(hipMalloc((void **)&pgm_ey, sizeof(cx<T>) * (int64_t)Wf * CN * H));
        if (!pgm_tiled) {
            // enter the tile-major regime: the two live iterates are re-laid out once
            need_natural(SPORCO_AMD_VAR_XF);   // (an ADMM leftover in the Xf buffer is resolved first)
            need_natural(SPORCO_AMD_VAR_YF);
            relayout(SPORCO_AMD_VAR_XF, true);
            relayout(SPORCO_AMD_VAR_YF, true);
            (void)cv(SPORCO_AMD_VAR_XFPRV);
            (void)cv(SPORCO_AMD_VAR_VF);
            // pgm_fft_momentum writes the new Xf and the new Yf at the same time: the new Xf goes
            // through the buffers of Xf / Xfprv / Vf in turn, the new Yf through those of Yf / Yfprv
            // -- the two Y buffers lie clear of the three X buffers (api_placement.inc)
            place_var(SPORCO_AMD_VAR_YFPRV, {SPORCO_AMD_VAR_XF, SPORCO_AMD_VAR_XFPRV, SPORCO_AMD_VAR_VF}, "Yfprv");
            place_var(SPORCO_AMD_VAR_YF, {SPORCO_AMD_VAR_XF, SPORCO_AMD_VAR_XFPRV, SPORCO_AMD_VAR_VF}, "Yf");
            place_release_spares();
            // (hold == 2: the previous Yf is state -- the residual of this iteration compares with it)
            if (p.hold == 2) relayout(SPORCO_AMD_VAR_YFPRV, true);
            pgm_tiled = true;
        }
        if (pgm_x_stale) pgm_x_stale = false;   // X of the previous iteration is superseded
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF), *Yf = cv(SPORCO_AMD_VAR_YF);
        cx<T> *Xprv = cv(SPORCO_AMD_VAR_XFPRV), *Yprv = cv(SPORCO_AMD_VAR_YFPRV);
        (void)Xprv;      // (touched for its allocation: the rotation below goes through the variable ids)
        cx<T> *spare = cv(SPORCO_AMD_VAR_VF), *Tm = work_buf();
        PgmColsArgs<T> ca;
        ca.dft = dft;
        ca.sft = sft;
        ca.twA = twA;
        ca.twB = twB;
        ca.inv_L = (T)(1.0 / p.L);
        ca.beta = (T)p.beta;
        ca.H = H;
        ca.W = W;
        ca.CN = CN;
        ca.K = K;
        ca.want_stats = p.want_stats || p.hold;
        ca.ey = p.hold ? pgm_ey : nullptr;
        // 1. gradient step at Yf, inverse transform along H
        ca.yf = Yf;
        ca.xf_old = nullptr;
        ca.t = Tm;
        ca.yf_new = nullptr;
        ca.partials = part_f;
        int64_t ntile;
        if (NHp > 1) {
            // K > 64: cooperating slab workgroups (csc_fused.h launch_pgm_grad_slabs)
            FusedSlabArgs<T> sa;
            sa.c.t = Tm;
            sa.c.dft = dft;
            sa.c.sft = sft;
            sa.c.twA = twA;
            sa.c.twB = twB;
            sa.c.H = H;
            sa.c.W = W;
            sa.c.CN = CN;
            sa.c.K = K;
            sa.c.partials = part_f;
            sa.qpart = qpart;
            sa.pgm_yf = Yf;
            sa.pgm_inv_L = ca.inv_L;
            sa.pgm_ey = ca.ey;
            coop_prepare(sa);
            ProfScope ps(prof, PS_PGM_GRAD_IFFT);
            ntile = launch_pgm_grad_slabs<T>(st, sa);
        } else {
            if (dmask) {
                // The residual at Yf through the mask; the gradient kernel takes it from memory.
                // e is affine in its argument and Yf = Xf + beta (Xf - Xf_prev), so from the third
                // iteration of a run on R(Yf) = (1 + beta) R(Xf) - beta R(Xf_prev) is formed from the
                // two signal-sized residuals kept from the previous calls instead of another
                // pass over the spectrum.
                const int64_t ns = (int64_t)H * W * CNs;
                if (!pgm_rx[0]) {
                    SA_HIP(hipMalloc((void **)&pgm_rx[0], sizeof(T) * ns));
                    SA_HIP(hipMalloc((void **)&pgm_rx[1], sizeof(T) * ns));
                }
                if (pgm_rx_count >= 2) {
                    const T bprev = (T)last_pgm.beta;
                    ProfScope ps(prof, PS_PGM);
                    launch_axpby<T>(st, T(1) + bprev, pgm_rx[pgm_rx_cur], -bprev, pgm_rx[pgm_rx_cur ^ 1],
                                    sreal, ns);
                } else {
                    pgm_resid_spatial(Yf, sreal);
                }
                pgm_masked_to_spectrum(pgm_ey);
                ca.ey_in = pgm_ey;
            }
            ProfScope ps(prof, PS_PGM_GRAD_IFFT);
            ntile = launch_pgm_grad_ifft<T>(st, ca);
            ca.ey_in = nullptr;
        }
        if (!dmask) {
            const int slots[1] = {SPORCO_AMD_PGM_FY};
            const double scales[1] = {0.5};
            finalize(part_f, (int)ntile, 1, 1, slots, scales, out_dev);
        }
        // 2. inverse along W, proximal map, forward along W
        pgm_rows_prox(p, Tm, spare, nullptr, out_dev);
        // 3. forward along H (in place: `spare` becomes the new Xf), momentum into the old
        //    Yfprv buffer, residual and objective sums
        ca.yf = Yf;
        ca.xf_old = Xf;
        ca.t = spare;
        // (hold == 2: a rule that forms Yf itself -- no momentum output, and the buffer of
        // VAR_YFPRV keeps the previous Yf)
        ca.yf_new = p.hold == 2 ? nullptr : Yprv;
        ca.partials = part_pgm;
        const bool stats_req = ca.want_stats;
        if (dmask) ca.want_stats = 0;     // (the kernel's own sums are the unmasked objective)
        ca.qpart = (NHp > 1 && ca.want_stats) ? qpart : nullptr;
        int64_t nrows;
        {
            ProfScope ps(prof, PS_PGM_FFT_MOM);
            nrows = launch_pgm_fft_momentum<T>(st, ca);
        }
        if (NHp > 1) {
            // per (tile, slab): the residual sums; per tile, from the slabs' shares: the objective
            const int s0[1] = {SPORCO_AMD_PGM_RSDL}, s4[1] = {SPORCO_AMD_PGM_DXY2};
            const double c0[1] = {1.0 / ((double)H * W)}, c4[1] = {1.0};
            finalize(part_pgm, (int)nrows, kPgmPartialStride, 1, s0, c0, out_dev);
            if (p.hold) finalize(part_pgm + 4, (int)nrows, kPgmPartialStride, 1, s4, c4, out_dev);
            if (ca.want_stats) {
                {
                    ProfScope ps(prof, PS_PGM_FFT_MOM);
                    launch_pgm_stats_slabs<T>(st, ca, part_pgm2);
                }
                const int s2[3] = {SPORCO_AMD_PGM_DFID, SPORCO_AMD_PGM_F, SPORCO_AMD_PGM_LIN};
                const double c2[3] = {1.0 / ((double)H * W), 0.5, 1.0};
                finalize(part_pgm2, (int)ntile, 3, p.hold ? 3 : 2, s2, c2, out_dev);
            }
        } else {
            const int slots[5] = {SPORCO_AMD_PGM_RSDL, SPORCO_AMD_PGM_DFID, SPORCO_AMD_PGM_F,
                                  SPORCO_AMD_PGM_LIN, SPORCO_AMD_PGM_DXY2};
            const double scales[5] = {1.0 / ((double)H * W), 1.0 / ((double)H * W), 0.5, 1.0, 1.0};
            finalize(part_pgm, (int)ntile, kPgmPartialStride, p.hold ? 5 : ca.want_stats ? 3 : 1, slots,
                     scales, out_dev);
        }
        if (dmask) {
            // the residual at the new Xf (in `spare` until the commit below): the next gradient's
            // input (above) and, weighted by W, the masked objective (pgm/cbpdn.py:481-489)
            const int64_t ns = (int64_t)H * W * CNs;
            pgm_rx_cur ^= 1;
            pgm_resid_spatial(spare, pgm_rx[pgm_rx_cur]);
            pgm_rx_count = pgm_rx_count < 2 ? pgm_rx_count + 1 : 2;
            if (stats_req) {
                SA_HIP(hipMemcpyAsync(sreal, pgm_rx[pgm_rx_cur], sizeof(T) * ns, hipMemcpyDeviceToDevice, st));
                int nb;
                {
                    ProfScope ps(prof, PS_PGM);
                    nb = launch_mask_apply<T>(st, sreal, have_wdat ? wdat : Weight<T>(), false, H, W, Cs, N,
                                              part_a);
                }
                const int slots[1] = {SPORCO_AMD_PGM_DFID};
                const double scales[1] = {1.0};
                finalize(part_a, nb, 1, 1, slots, scales, out_dev);
            }
        } else {
            pgm_rx_count = 0;
        }
        last_pgm = p;
        pgm_held = true;
        pgm_hold_kind = p.hold;
        if (!p.hold) pgm_commit();
    }

    // on_iteration_start's copies as a rotation of buffers (pgm.py:835-846): the trial in the
    // spare buffers becomes the state
    int pgm_hold_kind = 0;
    void pgm_commit() override {
        SA_REQUIRE(pgm_held, "pgm_commit without a held pgm_iter");
        pgm_held = false;
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF), *Yf = cv(SPORCO_AMD_VAR_YF);
        cx<T> *Xprv = cv(SPORCO_AMD_VAR_XFPRV), *Yprv = cv(SPORCO_AMD_VAR_YFPRV);
        cx<T> *spare = cv(SPORCO_AMD_VAR_VF);
        vars[SPORCO_AMD_VAR_XF] = spare;
        vars[SPORCO_AMD_VAR_XFPRV] = Xf;
        vars[SPORCO_AMD_VAR_VF] = Xprv;
        vars[SPORCO_AMD_VAR_YF] = Yprv;
        vars[SPORCO_AMD_VAR_YFPRV] = Yf;
        xf_tiled = false;
        x_stale = false;
        x_invalid = false;
        pgm_x_stale = true;
    }

    void pgm_grad(int var, double *out_dev) override {
        require_ready();
        SA_REQUIRE(var_is_complex(var), "pgm_grad needs a frequency-domain variable");
        before_read(var);
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            nb = Cd > 1 ? launch_mc_pgm_grad<T>(st, cv(var), cv(SPORCO_AMD_VAR_DF),
                                                cv(SPORCO_AMD_VAR_SF), cv(SPORCO_AMD_VAR_GF), npix,
                                                Cd, N, K, W, part_a)
                        : launch_pgm_grad<T>(st, cv(var), cv(SPORCO_AMD_VAR_DF),
                                             cv(SPORCO_AMD_VAR_SF), cv(SPORCO_AMD_VAR_GF), npix, CN,
                                             K, W, part_a);
        }
        const int slots[2] = {SPORCO_AMD_PGM_F, SPORCO_AMD_PGM_DFID};
        const double scales[2] = {0.5, 1.0 / ((double)H * W)};
        finalize(part_a, nb, 2, 2, slots, scales, out_dev);
    }

    void pgm_eval(int var, double *out_dev) override {
        require_ready();
        SA_REQUIRE(var_is_complex(var), "pgm_eval needs a frequency-domain variable");
        before_read(var);
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            inner_df(cv(var));
            nb = launch_pair_stats<T>(st, innerb, cv(SPORCO_AMD_VAR_SF), nullptr, npix, CNs, W, part_a);
        }
        // partial layout per block: [0] weighted |d|^2, [1] Re<d,g>, [2] |d|^2, [3] |g|^2
        const int s0[1] = {SPORCO_AMD_PGM_DFID};
        const double c0[1] = {1.0 / ((double)H * W)};
        finalize(part_a, nb, 4, 1, s0, c0, out_dev);
        const int s2[1] = {SPORCO_AMD_PGM_F};
        const double c2[1] = {0.5};
        finalize(part_a + 2, nb, 4, 1, s2, c2, out_dev);
        {
            ProfScope ps(prof, PS_PGM);
            nb = launch_pair_stats<T>(st, innerb, nullptr, nullptr, npix, CNs, W, part_b);
        }
        const int s3[1] = {SPORCO_AMD_PGM_HESS};
        const double c3[1] = {1.0};
        finalize(part_b + 2, nb, 4, 1, s3, c3, out_dev);
    }

    void pgm_prox_step(double L, double lmbda, uint32_t flags, int dH, int dW,
                       double *out_dev) override {
        require_ready();
        pgm_leave_tiled();
        x_written();
        cx<T> *Vf = cv(SPORCO_AMD_VAR_VF);
        {
            ProfScope ps(prof, PS_PGM);
            launch_axpy_c<T>(st, cv(SPORCO_AMD_VAR_YF), cv(SPORCO_AMD_VAR_GF), Vf, (T)(-1.0 / L), EF);
        }
        T *X = rv(SPORCO_AMD_VAR_X);
        inv2(Vf, work_buf(), X, P);
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            nb = launch_prox_l1<T>(st, X, X, (T)(lmbda / L), flags, d5(), dH, dW, wl1, part_b);
        }
        const int slots[1] = {SPORCO_AMD_PGM_L1};
        const double scales[1] = {1.0};
        finalize(part_b, nb, 1, 1, slots, scales, out_dev);
        xf_tiled = false;
        fwd2(X, nullptr, T(0), cv(SPORCO_AMD_VAR_XF), P);
    }

    void lincomb(int dst, double a, int va, double b, int vb, double c, int vc) override {
        SA_REQUIRE(var_is_valid(dst) && var_is_complex(dst) && dst != SPORCO_AMD_VAR_SF,
                   "lincomb works on frequency-domain state variables");
        for (int v : {va, vb, vc})
            SA_REQUIRE(v < 0 || (var_is_complex(v) && var_bytes(v) == var_bytes(dst)),
                       "lincomb operand of the wrong kind");
        SA_REQUIRE(va >= 0, "lincomb needs a first operand");
        if ((dst == SPORCO_AMD_VAR_YF || aux_slot(dst) >= 0) && tiled_operands({dst, va, vb, vc})) {
            // between fused iterations (pgm_iter): the combination is formed in the tile-major
            // layout the iterates are in (elementwise: any common layout will do) -- the Yf of
            // robust backtracking, its Z update, the monotone restart
            for (int v : {va, vb, vc})
                if (v >= 0) aux_to_tiled(v);
            if (aux_slot(dst) >= 0) {
                (void)cv(dst);
                aux_tiled[aux_slot(dst)] = true;
            }
            ProfScope ps(prof, PS_PGM);
            launch_lincomb<T>(st, cv(dst), (T)a, cv(va), (T)b, vb >= 0 ? cv(vb) : nullptr, (T)c,
                              vc >= 0 ? cv(vc) : nullptr, EF);
            return;
        }
        if (is_pgm_iterate(dst)) pgm_leave_tiled();
        for (int v : {va, vb, vc})
            if (v >= 0) before_read(v);
        if (dst == SPORCO_AMD_VAR_XF) xf_tiled = false;
        aux_written_natural(dst);
        ProfScope ps(prof, PS_PGM);
        launch_lincomb<T>(st, cv(dst), (T)a, cv(va), (T)b, vb >= 0 ? cv(vb) : nullptr, (T)c,
                          vc >= 0 ? cv(vc) : nullptr, (int64_t)(var_bytes(dst) / sizeof(cx<T>)));
    }

    // ---- residual spectra for the step-size policies (sporco/pgm/stepsize.py:67-145) ---------
    // e = sum_m Df v - Sf of an X-sized spectrum `var`, signal sized, kept tile-major in one of
    // four slots: the gradient conj(Df) e and its products follow from it (pgm_resid_stats)
    // without an X-sized gradient array.  One read pass over `var`.
    cx<T> *pgm_es[4] = {nullptr, nullptr, nullptr, nullptr};
    void pgm_resid(int var, int slot) override {
        require_single_channel_dict();
        require_ready();
        SA_REQUIRE(slot >= 0 && slot < 4, "residual slot out of range");
        SA_REQUIRE(var_is_valid(var) && var_is_complex(var) && !var_is_dict_sized(var) &&
                       var != SPORCO_AMD_VAR_SF && var != SPORCO_AMD_VAR_DF,
                   "pgm_resid needs an X-sized frequency-domain variable");
        SA_REQUIRE(fused || fused_slabs, "pgm_resid: shape not served by the fused kernels");
        const int64_t ntile = (int64_t)Wf * CN;
        if (!pgm_es[slot]) SA_HIP(hipMalloc((void **)&pgm_es[slot], sizeof(cx<T>) * ntile * H));
        ProfScope ps(prof, PS_PGM);
        if (pgm_tiled && is_pgm_iterate(var) && Ks == K) {
            launch_tiled_resid<T>(st, cv(var), dft, sft, pgm_es[slot], ntile, H, K, Ks, CN);
            return;
        }
        before_read(var);
        launch_inner<T>(st, cv(SPORCO_AMD_VAR_DF), cv(var), innerb, npix, CN, K);
        launch_lincomb<T>(st, innerb, T(1), innerb, T(-1), cv(SPORCO_AMD_VAR_SF), T(0), nullptr, npix * CN);
        launch_permute_ab<cx<T>>(st, innerb, pgm_es[slot], H, ntile, 1);          // -> (Wf CN, H)
    }
    void pgm_resid_stats(int a, int b, int c, int d, double *out_dev) override {
        SA_REQUIRE(a >= 0 && a < 4 && pgm_es[a], "pgm_resid_stats: first slot not filled");
        for (int s : {b, c, d})
            SA_REQUIRE(s < 0 || (s < 4 && pgm_es[s]), "pgm_resid_stats: slot not filled");
        SA_REQUIRE(d < 0 || c >= 0, "pgm_resid_stats: d without c");
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            nb = launch_resid_stats<T>(st, pgm_es[a], b >= 0 ? pgm_es[b] : nullptr,
                                       c >= 0 ? pgm_es[c] : nullptr, d >= 0 ? pgm_es[d] : nullptr, gramt,
                                       (int64_t)Wf * CN, H, CN, part_a);
        }
        const int slots[3] = {0, 1, 2};
        const double scales[3] = {1.0, 1.0, 1.0};
        finalize(part_a, nb, 3, 3, slots, scales, out_dev);
    }

    void pair_stats(int va, int vb, int vg, double *out_dev) override {
        SA_REQUIRE(va >= 0 && var_is_valid(va) && var_is_complex(va) && va != SPORCO_AMD_VAR_SF,
                   "pair_stats needs a frequency-domain first operand");
        for (int v : {vb, vg})
            SA_REQUIRE(v < 0 || (var_is_complex(v) && var_bytes(v) == var_bytes(va)),
                       "pair_stats operands must have the same shape");
        const int64_t cols = var_is_dict_sized(va) ? KD() : P;
        // (iterates / scratch spectra while the iterates are tile-major: summed in that layout)
        const bool tiled = !var_is_dict_sized(va) && tiled_operands({va, vb, vg});
        for (int v : {va, vb, vg}) {
            if (v < 0) continue;
            if (tiled) aux_to_tiled(v);
            else before_read(v);
        }
        int nb;
        {
            ProfScope ps(prof, PS_PGM);
            nb = launch_pair_stats<T>(st, cv(va), vb >= 0 ? cv(vb) : nullptr,
                                      vg >= 0 ? cv(vg) : nullptr, npix, cols, W, part_a,
                                      tiled ? (int64_t)CN * H * K : 0);
        }
        const int slots[4] = {0, 1, 2, 3};
        const double scales[4] = {1.0 / ((double)H * W), 1.0, 1.0, 1.0};
        finalize(part_a, nb, 4, 4, slots, scales, out_dev);
    }

    void fft_var(int rvar, int cvar, bool inverse) override {
        SA_REQUIRE(var_is_valid(rvar) && var_is_valid(cvar) && !var_is_complex(rvar) &&
                       var_is_complex(cvar) && cvar != SPORCO_AMD_VAR_SF &&
                       var_is_dict_sized(rvar) == var_is_dict_sized(cvar),
                   "fft_var needs a real and a complex variable of matching shape");
        const int64_t cols = var_is_dict_sized(rvar) ? KD() : P;
        if (is_pgm_iterate(cvar)) pgm_leave_tiled();
        if (inverse) {
            before_read(cvar);
            if (rvar == SPORCO_AMD_VAR_X) x_written();
        } else {
            before_read(rvar);
            if (cvar == SPORCO_AMD_VAR_XF) xf_tiled = false;
        }
        if (inverse)
            inv2(cv(cvar), var_is_dict_sized(rvar) ? dwork_buf() : work_buf(), rv(rvar), cols);
        else
            fwd2(rv(rvar), nullptr, T(0), cv(cvar), cols);
    }
