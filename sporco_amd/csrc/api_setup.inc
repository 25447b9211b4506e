// api_setup.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): set_signal / set_dict / weights / upload / download / queries.
    // ---- set-up ------------------------------------------------------------------
    void set_signal(const void *S) override {
        before_state_change();
        SA_HIP(hipMemcpyAsync(sreal, S, sizeof(T) * (int64_t)H * W * CNs, hipMemcpyHostToDevice, st));
        fwd2(sreal, nullptr, T(0), cv(SPORCO_AMD_VAR_SF), CNs);
        if (cplx_pair) pm_pair(cv(SPORCO_AMD_VAR_SF), cv(SPORCO_AMD_VAR_SF), 1, N, 1);
        refresh_fused_signal();
        sync();  // the host buffer may be released after return
        have_signal = true;
    }

    void set_signal_dev(const void *S_dev) override {
        before_state_change();
        SA_HIP(hipMemcpyAsync(sreal, S_dev, sizeof(T) * (int64_t)H * W * CNs,
                              hipMemcpyDeviceToDevice, st));
        fwd2(sreal, nullptr, T(0), cv(SPORCO_AMD_VAR_SF), CNs);
        if (cplx_pair) pm_pair(cv(SPORCO_AMD_VAR_SF), cv(SPORCO_AMD_VAR_SF), 1, N, 1);
        refresh_fused_signal();
        sync();
        have_signal = true;
    }

    void set_dict(const void *D, int dH, int dW) override {
        SA_REQUIRE(dH >= 1 && dW >= 1 && dH <= H && dW <= W,
                   "filter support must fit inside the signal");
        before_dict_change();
        if (!dpad) SA_HIP(hipMalloc((void **)&dpad, sizeof(T) * (int64_t)H * W * Cd * K));
        // stage the compact filters at the tail of dpad's own allocation? no: use `work`-free
        // dedicated staging so set_dict is safe while iterates are live.
        T *stage = nullptr;
        SA_HIP(hipMalloc((void **)&stage, sizeof(T) * (int64_t)dH * dW * Cd * Ku));
        SA_HIP(hipMemcpyAsync(stage, D, sizeof(T) * (int64_t)dH * dW * Cd * Ku, hipMemcpyHostToDevice,
                              st));
        {   // (Cd > 1: host layout (dH, dW, Cd, K), never padded)
            ProfScope ps(prof, PS_OTHER);
            launch_pad_dict<T>(st, stage, dpad, H, W, Cd * K, dH, dW, Cd * Ku);
        }
        fwd2(dpad, nullptr, T(0), cv(SPORCO_AMD_VAR_DF), (int64_t)Cd * K);
        ism_valid = false;
        if (Cd == 1) {
            ProfScope ps(prof, PS_OTHER);
            launch_gram<T>(st, cv(SPORCO_AMD_VAR_DF), gram, npix, K);
        }
        refresh_fused_dict();
        sync();
        SA_HIP(hipFree(stage));
        dH_ = dH;
        dW_ = dW;
        have_dict = true;
    }

    // The imaginary part of a complex dictionary (the real part goes through set_dict): switches
    // the handle to complex mode -- the caller's signal, dictionary and coefficient maps are
    // complex, their real / imaginary parts the channel halves of this (even-C) handle
    // (sporco/admm/cbpdn.py:209-217, :242-256).  D == null: back to a real dictionary.
    void set_dict_imag(const void *D, int dH, int dW) override {
        before_dict_change();
        if (!D) {
            cplx = false;
            return;
        }
        SA_REQUIRE(Cd == 1 && C % 2 == 0,
                   "complex mode: single-channel dictionary, real / imaginary channel halves");
        SA_REQUIRE(dH >= 1 && dW >= 1 && dH <= H && dW <= W, "filter support must fit inside the signal");
        if (!dpad) SA_HIP(hipMalloc((void **)&dpad, sizeof(T) * (int64_t)H * W * Cd * K));
        if (!df_im) SA_HIP(hipMalloc((void **)&df_im, sizeof(cx<T>) * npix * K));
        T *stage = nullptr;
        SA_HIP(hipMalloc((void **)&stage, sizeof(T) * (int64_t)dH * dW * Ku));
        SA_HIP(hipMemcpyAsync(stage, D, sizeof(T) * (int64_t)dH * dW * Ku, hipMemcpyHostToDevice, st));
        {
            ProfScope ps(prof, PS_OTHER);
            launch_pad_dict<T>(st, stage, dpad, H, W, K, dH, dW, Ku);
        }
        fwd2(dpad, nullptr, T(0), df_im, (int64_t)K);
        sync();
        SA_HIP(hipFree(stage));
        cplx = true;
    }

    void set_weight(int which, const void *w, const int64_t shape[5]) override {
        before_state_change();   // a pending X of the fused PGM step depends on the weights
        if (which == 2) ams_bits_valid = false;
        if (which == 3) have_wdat = w != nullptr;
        if (which == 0) inhib_drop();   // (the L1-weight array held the inhibition thresholds)
        Weight<T> &dst = which == 0 ? wl1 : (which == 1 ? wl21 : (which == 2 ? wams : wdat));
        T *&buf = which == 0 ? wl1_buf : (which == 1 ? wl21_buf : (which == 2 ? wams_buf : wdat_buf));
        if (buf) {
            sync();
            SA_HIP(hipFree(buf));
            buf = nullptr;
        }
        dst = Weight<T>();
        if (!w) return;
        // (the data-fidelity mask lives on the signal, which keeps its channels under a
        // multi-channel dictionary)
        const int64_t full[5] = {H, W, which == 3 ? Cs : C, N, Ku};
        int64_t n = 1;
        // (the AddMaskSim mask of a multi-channel dictionary has one slice per impulse filter
        // on its last axis: cbpdn.py:2358-2364 swaps the mask's channel axis there)
        const bool ams_mc = which == 2 && Cd > 1 && shape[4] == Cd;
        for (int i = 0; i < 5; ++i) {
            SA_REQUIRE(shape[i] == 1 || shape[i] == full[i] || (i == 4 && ams_mc),
                       "weight shape must be 1 or the full extent on every axis");
            n *= shape[i];
        }
        if (which == 1) SA_REQUIRE(shape[2] == 1, "L21Weight must not vary over the channel axis");
        if (which >= 2)
            SA_REQUIRE(shape[4] == 1 || ams_mc, "the mask must not vary over the filter axis");
        int64_t dshape[5] = {shape[0], shape[1], shape[2], shape[3], shape[4]};
        std::vector<T> padded;
        const void *srcp = w;
        if (K != Ku && shape[4] == Ku && !ams_mc) {
            // weight 1 on the padding filter (its coefficients are zero whatever the weight)
            dshape[4] = K;
            const int64_t rows = n / Ku;
            padded.assign((size_t)(rows * K), T(1));
            const T *wt = static_cast<const T *>(w);
            for (int64_t r = 0; r < rows; ++r)
                for (int k = 0; k < Ku; ++k) padded[(size_t)(r * K + k)] = wt[r * Ku + k];
            srcp = padded.data();
            n = rows * K;
        }
        SA_HIP(hipMalloc((void **)&buf, sizeof(T) * n));
        SA_HIP(hipMemcpyAsync(buf, srcp, sizeof(T) * n, hipMemcpyHostToDevice, st));
        sync();
        int64_t stride = 1;
        for (int i = 4; i >= 0; --i) {
            dst.stride[i] = dshape[i] == 1 ? 0 : stride;
            stride *= dshape[i];
        }
        dst.ptr = buf;
    }

    // GradWeight (cbpdn.py:1063-1071, :1134-1139): K per-filter weights, NULL => scalar 1
    void set_grad_weight(const void *w) override {
        before_state_change();
        have_wg = w != nullptr;
        g1_valid = false;
        ism_valid = false;
        if (!w) return;
        if (!wg) SA_HIP(hipMalloc((void **)&wg, sizeof(T) * K));
        std::vector<T> tmp((size_t)K, T(1));
        std::memcpy(tmp.data(), w, sizeof(T) * Ku);
        SA_HIP(hipMemcpyAsync(wg, tmp.data(), sizeof(T) * K, hipMemcpyHostToDevice, st));
        SA_HIP(hipStreamSynchronize(st));
    }

    // sum_i |G_i|^2 of the difference filters [1, -1] along each axis is separable:
    // |1 - e^{-i t}|^2 = 2 - 2 cos t  (signal.gradient_filters, signal.py:230-239)
    GradTerm<T> grad_term(double mu) {
        if (!ghh) {
            std::vector<T> th(H), tw(Wf);
            const double tau = 6.283185307179586476925286766559;
            for (int h = 0; h < H; ++h) th[h] = (T)(2.0 - 2.0 * std::cos(tau * h / H));
            for (int f = 0; f < Wf; ++f) tw[f] = (T)(2.0 - 2.0 * std::cos(tau * f / W));
            // a singleton axis crops the 2-tap filter to its first tap (numpy's fft `s` rule)
            if (H == 1) th[0] = T(1);
            if (W == 1) tw[0] = T(1);
            SA_HIP(hipMalloc((void **)&ghh, sizeof(T) * H));
            SA_HIP(hipMalloc((void **)&ghw, sizeof(T) * Wf));
            SA_HIP(hipMemcpy(ghh, th.data(), sizeof(T) * H, hipMemcpyHostToDevice));
            SA_HIP(hipMemcpy(ghw, tw.data(), sizeof(T) * Wf, hipMemcpyHostToDevice));
        }
        GradTerm<T> g;
        g.ghh = ghh;
        g.ghw = ghw;
        g.wg = have_wg ? wg : nullptr;
        g.mu = (T)mu;
        return g;
    }

    // Host <-> device copy of one state array; the host side has Ku filters on its last axis.
    void host_copy(int var, void *host, bool to_device) {
        void *dev = var_ptr(var);
        const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        if (K == Ku || var == SPORCO_AMD_VAR_SF || var_is_signal_real(var) || var_is_rtv_grad(var)) {
            if (to_device) SA_HIP(hipMemcpyAsync(dev, host, var_bytes(var), kind, st));
            else SA_HIP(hipMemcpyAsync(host, dev, var_bytes(var), kind, st));
            return;
        }
        const size_t es = var_is_complex(var) ? sizeof(cx<T>) : sizeof(T);
        const size_t rows = var_bytes(var) / (es * K);
        if (to_device) {
            SA_HIP(hipMemsetAsync(dev, 0, var_bytes(var), st));
            SA_HIP(hipMemcpy2DAsync(dev, es * K, host, es * Ku, es * Ku, rows, kind, st));
        } else {
            SA_HIP(hipMemcpy2DAsync(host, es * Ku, dev, es * K, es * Ku, rows, kind, st));
        }
    }

    void upload(int var, const void *src) override {
        if (is_pgm_iterate(var)) pgm_leave_tiled();
        aux_written_natural(var);
        if (var == SPORCO_AMD_VAR_ZF) {
            zf_tiled = false;
            gramz_valid = false;
            zsf_valid = dism_valid = zfv_valid = false;
        }
        if (var == SPORCO_AMD_VAR_X) {
            x_written();
        } else if (var == SPORCO_AMD_VAR_XF) {
            if ((x_stale && !x_invalid) || md_x_pending) materialize_x();   // keep X; Xf is replaced below
        } else if (var == SPORCO_AMD_VAR_Y || var == SPORCO_AMD_VAR_U || var == SPORCO_AMD_VAR_DF ||
                   var == SPORCO_AMD_VAR_SF) {
            before_state_change();
        }
        host_copy(var, const_cast<void *>(src), true);
        if (var == SPORCO_AMD_VAR_XF) xf_tiled = false;
        if (var == SPORCO_AMD_VAR_DF) {
            ism_valid = false;
            if (Cd == 1) launch_gram<T>(st, cv(SPORCO_AMD_VAR_DF), gram, npix, K);
            refresh_fused_dict();
        }
        if (var == SPORCO_AMD_VAR_SF) refresh_fused_signal();
        sync();
    }
    void download(int var, void *dst) override {
        if (var == SPORCO_AMD_VAR_YPREV || var == SPORCO_AMD_VAR_AX) ensure_prev_yu();
        if (it.prev_at == PrevAt::AltYU && y_alt && (var == SPORCO_AMD_VAR_YPREV || var == SPORCO_AMD_VAR_AX)) {
            // Yprev = the other half of the (Y, U) ping-pong; AX = rlx X + (1 - rlx) Yprev
            // (admm.py:877-885) with X rebuilt from that same previous iterate
            if (var == SPORCO_AMD_VAR_YPREV) {
                SA_HIP(hipMemcpyAsync(rv(var), y_alt, sizeof(T) * E, hipMemcpyDeviceToDevice, st));
            } else {
                materialize_x();
                ProfScope ps(prof, PS_OTHER);
                launch_relax<T>(st, rv(SPORCO_AMD_VAR_X), y_alt, rv(SPORCO_AMD_VAR_AX),
                                (T)last_p.rlx, E);
            }
        }
        before_read(var);
        host_copy(var, dst, false);
        sync();
    }
    void *device_ptr(int var) override {
        before_read(var);
        return var_ptr(var);
    }

    void read_out(const double *out_dev, double *out_host) override {
        SA_HIP(hipMemcpyAsync(out_pinned, out_dev, sizeof(double) * kOutSlots, hipMemcpyDeviceToHost,
                              st));
        sync();
        std::memcpy(out_host, out_pinned, sizeof(double) * kOutSlots);
    }

    void require_single_channel_dict() const {
        if (Cd > 1)
            throw Error(SPORCO_AMD_EINVAL,
                        "multi-channel dictionaries are handled by the ADMM ConvBPDN calls only");
    }
    void require_ready() const {
        if (!have_dict || !have_signal)
            throw Error(SPORCO_AMD_ESTATE, "set_signal and set_dict must be called first");
    }

    // column FFT + Sherman-Morrison + column IFFT on the tile-major spectrum in the
    // Xf buffer (csc_fused.h); the data-fidelity sum goes to out_dev when wanted
    // (striped: the output goes to cols_out[] instead of back into the Xf buffer, csc_fused.h)
    bool run_fused_cols(const sporco_amd_admm_params &p, double *out_dev, bool striped = false) {
        if (fused_mc) {
            SA_REQUIRE(!(p.flags & (F_GRADREG | F_AMS | F_JOINT)),
                       "this solver variant needs a single-channel dictionary");
            if (!binv_valid || binv_rho != p.rho) {
                ProfScope ps(prof, PS_OTHER);
                launch_mc_binv<T>(st, dft_mc, bt_mc, npix, Cd, K, (T)p.rho);
                binv_valid = true;
                binv_rho = p.rho;
            }
            FusedMcArgs<T> ma;
            ma.t = cv(SPORCO_AMD_VAR_XF);
            ma.dft = dft_mc;
            ma.sft = sft_mc;
            ma.bt = bt_mc;
            ma.twA = twA;
            ma.twB = twB;
            ma.rho = (T)p.rho;
            ma.H = H;
            ma.W = W;
            ma.N = N;
            ma.K = K;
            ma.Cd = Cd;
            ma.partials = part_f;
            int64_t nt;
            {
                ProfScope ps(prof, PS_FUSED_COLS);
                nt = launch_fused_cols_mc<T>(st, ma);
            }
            part_f_rows = (int)nt;
            xf_tiled = true;
            if (out_dev && (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y)) {
                const int slots[1] = {SPORCO_AMD_OUT_DFID};
                const double scales[1] = {1.0 / ((double)H * W)};
                finalize(part_f, (int)nt, 1, 1, slots, scales, out_dev);
            }
            return false;
        }
        const bool gradreg = p.flags & F_GRADREG;
        // (striped: the single K <= 64 kernel without the gradient term only)
        striped = striped && cols_striped() && !gradreg && !tail_mode && !fused_slabs;
        auto fa = fused_cols_args(p.rho, striped);
        if (gradreg) {
            SA_REQUIRE(fused || fused_slabs, "no gradient-regularised column pass for this shape");
            const GradTerm<T> gt = grad_term(p.mu);
            if (!g1t) SA_HIP(hipMalloc((void **)&g1t, sizeof(T) * npix));
            fa.ghh = gt.ghh;
            fa.ghw = gt.ghw;
            fa.wg = gt.wg;
            fa.mu = gt.mu;
            fa.g1t_out = g1t;
            if (!g1_valid || g1_rho != p.rho || g1_mu != p.mu) {
                ProfScope ps(prof, PS_OTHER);
                launch_grad_g1<T>(st, fa);
                g1_valid = true;
                g1_rho = p.rho;
                g1_mu = p.mu;
            }
            fa.g1t = g1t;
        }
        int64_t ntiles;
        if (tail_mode) {
            // A handful of filters past 64 (the AddMaskSim impulse on a 64-filter dictionary):
            // they go through the generic column FFT, their inner products are folded into
            // Sf, and the register-resident kernel runs on the first 64 as if alone.
            if (!sft_eff) {
                SA_HIP(hipMalloc((void **)&sft_eff, sizeof(cx<T>) * npix * CN));
                SA_HIP(hipMalloc((void **)&coef_t, sizeof(cx<T>) * npix * CN));
            }
            const int Kt = K - 64;
            const int64_t nt = (int64_t)Wf * CN, tstride = (int64_t)H * Ks;
            cx<T> *tail = fa.t + 64;
            fa.Kv = 64;
            fa.coef_out = coef_t;
            ProfScope ps(prof, PS_FUSED_COLS);
            fft_c2c<T>(st, planH, false, tail, tail, nt, Kt, tstride, Ks, tstride, Ks, T(1));
            launch_tail_inner<T>(st, fa, sft, sft_eff);
            fa.sft = sft_eff;
            ntiles = launch_fused_cols<T>(st, fa);
            launch_tail_update<T>(st, fa);
            fft_c2c<T>(st, planH, true, tail, tail, nt, Kt, tstride, Ks, tstride, Ks, T(1));
        } else if (fused_slabs) {
            FusedSlabArgs<T> sa;
            sa.c = fa;
            sa.qpart = qpart;
            ProfScope ps(prof, PS_FUSED_COLS);
            ntiles = run_slab_cols(sa);
            if (gradreg) ntiles *= (K + 63) / 64;   // (one row of partials per tile and slab)
        } else {
            ProfScope ps(prof, PS_FUSED_COLS);
            ntiles = launch_fused_cols<T>(st, fa);
        }
        part_f_rows = (int)ntiles;
        xf_tiled = true;
        if (out_dev && (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y)) {
            const int slots[2] = {SPORCO_AMD_OUT_DFID, SPORCO_AMD_OUT_RGR};
            const double scales[2] = {1.0 / ((double)H * W), 1.0 / ((double)H * W)};
            const int nv = gradreg ? 2 : 1;
            finalize(part_f, (int)ntiles, nv, nv, slots, scales, out_dev);
        }
        return striped;
    }

    // One whole ADMM iteration in three launches (csc_rows.h): rows_fwd, fused_cols,
    // rows_inv_post.  X is written only on request (F_KEEP_X).
    void admm_iter_fused(const sporco_amd_admm_params &p, double *out_dev) {
        require_ready();
        const bool keep_x = p.flags & F_KEEP_X;
        const bool untouched = touch_epoch == fused_epoch;   // no host access since the last fused iteration
        if (!keep_x && !y_alt) alloc_alt_pair();      // (may move Y, U and the spectrum buffer)
        // Single-array state (csc_rows.h): from the second fused iteration in a row with no host
        // access to the iterates in between, the epilogue stores V' = AX + U alone and the next
        // iteration derives (Y, U) from it -- seven passes instead of ten (six instead of eight
        // with an emitted spectrum).  Anything else that wants Y or U gets them through
        // ensure_yu() (var_ptr).
        const VRoute vr = enter_iteration(p, untouched);
        T *const vin = vr.in.buf;
        T *Y = vin ? nullptr : rv(SPORCO_AMD_VAR_Y), *U = vin ? nullptr : rv(SPORCO_AMD_VAR_U);
        cx<T> *Xf = cv(SPORCO_AMD_VAR_XF);
        // rows_fwd, unless the previous iteration already left its result behind
        if (!(t_ready && p.u_scale == 1.0)) {
            if (vin) {
                auto ra = rows_fwd_args(vr.in, p);
                ra.s2 = (T)p.u_scale;
                run_rows_fwd(ra);
            } else {
                launch_rows_fwd_on(Y, U, (T)p.u_scale);
            }
        }
        t_ready = false;
        const bool striped = run_fused_cols(p, nullptr, !keep_x);
        // Bet on an unchanged rho only once it has stayed put for two updates in a row:
        // while AutoRho is still moving it almost every iteration a lost bet costs one
        // extra pass, a won one saves three (rows_fwd of the next iteration).
        stable_run = p.u_scale == 1.0 ? stable_run + 1 : 0;
        // (ConvBPDNJoint speculates too since round 3: its emitting epilogue used to spill the
        // tile -- 22.4 ms against 13.0 + 6.6 ms for epilogue + rows_fwd at config 3,
        // profiles/r02i_config3_*.json -- until the two elements of a pixel were serialised;
        // SPORCO_AMD_JOINT_EMIT=0 switches it off)
        const bool emit = stable_run >= 2 && !sw.no_speculation;
        auto pa = rows_post_args(p, striped);
        pa.t_next = emit ? Xf : nullptr;
        pa.y = Y;
        pa.u = U;
        pa.y_out = keep_x ? Y : y_alt;
        pa.u_out = keep_x ? U : u_alt;
        pa.v_in = vin;
        pa.v_out = vr.out;
        pa.thr_prev = vr.in.thr;
        pa.thr21_prev = vr.in.thr21;
        pa.x = keep_x ? rv(SPORCO_AMD_VAR_X) : nullptr;
        pa.thr = (T)(p.lmbda / p.rho);    // (the host's scalars; under ctl the control block's)
        pa.thr21 = (T)(p.mu / p.rho);
        pa.u_scale = (T)p.u_scale;
        int64_t nt;
        {
            ProfScope ps(prof, vin ? (emit ? PS_ROWS_INV_POST_V_EMIT : PS_ROWS_INV_POST_V)
                                   : (emit ? PS_ROWS_INV_POST_EMIT : PS_ROWS_INV_POST));
            nt = launch_rows_inv_post<T>(st, pa);
        }
        if (p.flags & (F_RESID | F_OBJ)) finalize_iter_sums(p, nt, out_dev);
        if (keep_x) {
            x_written();
        } else if (vr.out) {
            // the new iterate is the V in vr.out; the previous one is the V this iteration read, or
            // (first V iteration) the (Y, U) in vars
            const HeldV cur = held_v(p, vr.out, pa.thr, pa.thr21);
            commit_v(p, cur, vin ? &vr.in : nullptr);
        } else {
            commit_yu(p);     // the new iterate lives in the alternate buffers
        }
        t_ready = emit;
        if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) dfid_at(rv(SPORCO_AMD_VAR_Y), out_dev, &p);
        fused_epoch = touch_epoch;
    }
