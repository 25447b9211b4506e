// api_admm_run.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): the device-driven ADMM loop (sporco_amd_csc_admm_run).
    // ---- device-driven solve (include/sporco_amd.h: sporco_amd_csc_admm_run) -----------------
    bool admm_run_supported(const sporco_amd_admm_params &p) const {
        return !cplx && std::is_same<T, float>::value && rows_ok && mr_ok(p) && (fused || fused_slabs) && !fused_mc &&
               !tail_mode && !(p.flags & (F_XRRS | F_GRADREG | F_KEEP_X | F_FEVAL_Y)) &&
               (!(p.flags & F_JOINT) || joint_rows_ok(p)) && p.lmbda >= 0.0 && p.rho > 0.0 &&
               !std::getenv("SPORCO_AMD_HOST_LOOP");
    }

    // The run as one launch (csc_rows.h admm_persist): small problems, plain options, the
    // single-array state, no collective between the sums and the control update.  Opt-in
    // (SPORCO_AMD_PERSIST=1 or SPORCO_AMD_HINT_ONE_LAUNCH): it needs the whole device to itself
    // (its workgroups wait for each other), it buys 9-12 % where it applies
    // (profiles/r03_persist.md), and on the GPU its iterates equal those of the launch-per-pass
    // loop to rounding, not bit for bit.
    bool persist_ok(const sporco_amd_admm_params &p, const sporco_amd_admm_ctrl &c, bool vf,
                    bool has_reduce) const {
        const bool off = sw.persist >= 0 ? sw.persist != 1 : !hint_one_launch;
        return !off && vf && !has_reduce && fused && !fused_slabs && Ks == K && run_always_emit &&
               admm_persist_supported<T>(H, W, K) && !wl1.ptr && c.max_iter >= 3 &&
               !(p.flags & (F_NOBNDRY | F_AMS | F_JOINT)) && admm_persist_resident<T>(H, W, K, CN);
    }
    // (V form in and out, always emitting; every iteration-dependent scalar from the control block)
    PersistIterArgs<T> persist_iter_args(const sporco_amd_admm_params &p, T *vin, T *vout,
                                         double *prow, double *pcol) {
        PersistIterArgs<T> a;
        a.fwd = rows_fwd_args(held_v(p, vin, T(0), T(0)), p);
        a.fwd.s2 = T(1);
        a.cols = fused_cols_args(p.rho);
        a.cols.partials = pcol;
        a.post = rows_post_args(p);
        a.post.t_next = a.fwd.t;
        a.post.v_in = vin;
        a.post.v_out = vout;
        a.post.thr = T(0);      // (thr and u_scale: the control block's)
        a.post.u_scale = T(1);
        a.post.partials = prow;
        return a;
    }
    // iterations index0 .. max_iter - 1 of the run whose control block is ctl_dev; v_prev: the
    // iterate iteration index0 - 1 left, v_other: the other V buffer.  Returns how many ran.
    int run_persist(const sporco_amd_admm_params &p, int index0, int max_iter, T *v_prev, T *v_other,
                    bool want_sums) {
        const int grid = admm_persist_grid<T>(H, W, K, CN);
        const int64_t nrow = (int64_t)H * ceil_div(P, 128), ncol = (int64_t)Wf * CN;
        if (!pst_part_rows) {
            SA_HIP(hipMalloc((void **)&pst_part_rows, sizeof(double) * 8 * nrow));
            SA_HIP(hipMalloc((void **)&pst_part_f, sizeof(double) * 2 * ncol));
            SA_HIP(hipMalloc((void **)&pst_bar, sizeof(unsigned) * kPersistBarWords));
        }
        if (pst_grid < grid) {
            if (pst_blk) {
                sync();
                SA_HIP(hipFree(pst_blk));
                SA_HIP(hipFree(pst_ctl));
            }
            SA_HIP(hipMalloc(&pst_blk, sizeof(PersistIterArgs<T>) * 2 * grid));
            SA_HIP(hipMalloc((void **)&pst_ctl, sizeof(AdmmCtl) * grid));
            pst_grid = grid;
        }
        AdmmPersistArgs<T> a;
        // iteration j reads the V that iteration j - 1 wrote
        const int p0 = index0 & 1;
        a.iter[p0] = persist_iter_args(p, v_prev, v_other, part_rows, part_f);
        a.iter[p0 ^ 1] = persist_iter_args(p, v_other, v_prev, pst_part_rows, pst_part_f);
        a.blk = static_cast<PersistIterArgs<T> *>(pst_blk);
        a.ctl_blk = pst_ctl;
        a.ctl = ctl_dev;
        a.rec = reinterpret_cast<AdmmRecord *>(rec_ring) + index0;
        a.index0 = index0;
        a.max_iter = max_iter - index0;
        a.bar = pst_bar;
        a.n_row_tiles = (int)nrow;
        a.n_col_tiles = (int)ncol;
        a.want_dfid = (p.flags & F_OBJ) ? 1 : 0;
        a.want_sums = want_sums ? 1 : 0;
        a.dfid_scale = 1.0 / ((double)H * W);
        SA_HIP(hipMemsetAsync(pst_bar, 0, sizeof(unsigned) * kPersistBarWords, st));
        {
            ProfScope ps(prof, PS_PERSIST);
            launch_admm_persist<T>(st, a, grid);
        }
        unsigned bar[16];
        SA_HIP(hipMemcpyAsync(bar, pst_bar, sizeof(bar), hipMemcpyDeviceToHost, st));
        sync();
        if (bar[2]) throw Error(SPORCO_AMD_EHIP, "one-launch solve: a grid barrier did not complete");
        xf_tiled = true;
        ++pst_runs;
        return (int)bar[3];
    }

    // one iteration of admm_iter_fused with every iteration-dependent scalar taken from ctl_dev
    // vout set: the single-array state of csc_rows.h -- the iterate is read from vin (null: from
    // (Y, U), the first iteration of such a run) and V' is written to vout
    int64_t enqueue_iter_ctl(const sporco_amd_admm_params &p, T *vin = nullptr, T *vout = nullptr) {
        T *Y = vin ? nullptr : static_cast<T *>(vars[SPORCO_AMD_VAR_Y]);
        T *U = vin ? nullptr : static_cast<T *>(vars[SPORCO_AMD_VAR_U]);
        const bool striped = cols_striped() && !fused_slabs;
        {
            // (thresholds of a V input: the control block's)
            auto ra = vin ? rows_fwd_args(held_v(p, vin, T(0), T(0)), p) : rows_fwd_args();
            ra.y = Y;
            ra.u = U;
            ra.s2 = T(1);
            ra.ctl = ctl_dev;
            run_rows_fwd(ra);
        }
        {
            auto fa = fused_cols_args(p.rho, striped);
            fa.ctl = ctl_dev;
            ProfScope ps(prof, PS_FUSED_COLS);
            if (fused_slabs) {      // 64 < K <= 256: cooperating slab workgroups (csc_fused.h)
                FusedSlabArgs<T> sa;
                sa.c = fa;
                sa.qpart = qpart;
                part_f_rows = (int)run_slab_cols(sa);
            } else {
                part_f_rows = (int)launch_fused_cols<T>(st, fa);
            }
            xf_tiled = true;
        }
        auto pa = rows_post_args(p, striped);
        pa.y = Y;
        pa.u = U;
        pa.y_out = y_alt;
        pa.u_out = u_alt;
        pa.v_in = vin;
        pa.v_out = vout;
        pa.thr = T(0);          // (thr, u_scale and the previous thresholds: the control block's)
        pa.u_scale = T(1);
        pa.ctl = ctl_dev;
        // plain variant first, then the emitting one: ctl->emit picks
        int64_t nt = 0;
        if (!run_always_emit) {
            ProfScope ps(prof, vin ? PS_ROWS_INV_POST_V : PS_ROWS_INV_POST);
            nt = launch_rows_inv_post<T>(st, pa);
        }
        pa.t_next = cv(SPORCO_AMD_VAR_XF);
        {
            ProfScope ps(prof, vin ? PS_ROWS_INV_POST_V_EMIT : PS_ROWS_INV_POST_EMIT);
            nt = launch_rows_inv_post<T>(st, pa);
        }
        if (!vout) swap_alt_pair();
        return nt;
    }

    int admm_run(const sporco_amd_admm_params &p, const sporco_amd_admm_ctrl &c,
                 sporco_amd_admm_record *records, double *rho_out, double *u_scale_out,
                 sporco_amd_reduce_fn reduce, void *user) override {
        require_ready();
        if (!admm_run_supported(p)) return -1;
        SA_REQUIRE(c.max_iter >= 0, "max_iter must not be negative");
        if (c.max_iter == 0) {
            *rho_out = p.rho;
            *u_scale_out = p.u_scale;
            return 0;
        }
        if (!y_alt) alloc_alt_pair();
        // Single-array state (csc_rows.h) for runs of several iterations: the epilogue stores
        // V' = AX + U alone, rows_fwd and the next epilogue derive (Y, U) from it.  A run of a
        // few iterations (a dictionary-learning X-step) stays in the (Y, U) form: it would pay
        // the conversion back at once.
        const VRoute vr = enter_iteration(p, c.max_iter >= 4 || hint_vform);
        const bool vf = vr.out != nullptr;
        if (!ctl_dev) SA_HIP(hipMalloc((void **)&ctl_dev, sizeof(AdmmCtl)));
        if (rec_cap < c.max_iter) {
            if (rec_ring) SA_HIP(hipHostFree(rec_ring));
            rec_cap = std::max(c.max_iter, 256);
            SA_HIP(hipHostMalloc((void **)&rec_ring, sizeof(AdmmRecord) * rec_cap, 0));
        }
        std::memset((void *)rec_ring, 0, sizeof(AdmmRecord) * c.max_iter);
        double *out_dev = out_dev_default;
        const bool want_sums = p.flags & (F_RESID | F_OBJ);
        AdmmCtlInit in;
        in.rho = p.rho;
        in.u_scale = p.u_scale;
        in.lmbda = p.lmbda;
        in.abstol = c.abs_tol;
        in.reltol = c.rel_tol;
        in.sqrt_nc = c.sqrt_nc;
        in.sqrt_nx = c.sqrt_nx;
        in.tau = c.rho_tau;
        in.mu = c.rho_mu;
        in.xi = c.rho_xi;
        in.mu21 = p.mu;
        in.k = c.k0;
        in.stable_run = stable_run;
        in.emitted = t_ready ? 1 : 0;
        in.is_f32 = 1;
        in.autorho = c.auto_rho;
        in.period = c.period > 0 ? c.period : 1;
        in.autoscaling = c.auto_scaling;
        in.stdres = c.std_residuals;
        in.need_resid = c.need_residuals;
        in.thr_prev = (float)vr.in.thr;        // (zero when the run starts from (Y, U))
        in.thr21_prev = (float)vr.in.thr21;
        in.no_speculation = sw.no_speculation ? 1 : 0;
        // Small problems (kernels of a few microseconds): the emitting epilogue always, and its
        // plain twin is not enqueued at all -- a wasted emit costs less than a launch that
        // returns at once.
        run_always_emit = !in.no_speculation && E <= ((int64_t)1 << 22);
        if (run_always_emit) in.no_speculation = 2;
        launch_admm_ctl_init(st, ctl_dev, in);
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        const int ahead = c.lookahead > 0 ? c.lookahead : 3;
        int enq = 0, done = 0, stop_at = -1;
        // (test knob: pretend the newest `lag` records are not visible yet, so that launches
        // enqueued past the stopping iteration -- which must do nothing -- occur on any device)
        int lag = std::getenv("SPORCO_AMD_RUN_LAG") ? std::atoi(std::getenv("SPORCO_AMD_RUN_LAG")) : 0;
        // Advance `done` over finished iterations up to `upto` records: without `block` it
        // returns at the first unfinished one, with `block` it waits for each.
        auto poll = [&](int upto, bool block) {
            while (done < upto && stop_at < 0) {
                if (rec_ring[done].seq != done + 1) {
                    if (!block) return;
                    if (hipStreamQuery(st) == hipSuccess && rec_ring[done].seq != done + 1)
                        throw Error(SPORCO_AMD_EHIP, "device-driven solve: record not written");
                    continue;
                }
                if (rec_ring[done].stop) stop_at = done;
                ++done;
            }
        };
        T *vb_in = vr.in.buf;     // V form: input of the next enqueued iteration
        auto enqueue_one = [&]() {
            T *vb_out = vf ? other_alt(vb_in) : nullptr;
            const int64_t nt = enqueue_iter_ctl(p, vb_in, vb_out);
            vb_in = vb_out;
            if (want_sums) {
                // (no gradient term, data fidelity at X: admm_run_supported)
                finalize_iter_sums(p, nt, out_dev);
                if (reduce) reduce(user, out_dev);
                else if (comm_user) comm_reduce_sums(comm_user, out_dev, st);
            }
            launch_admm_ctl_update(st, ctl_dev, out_dev, rec_ring + enq, enq, true);
            ++enq;
        };
        // Iteration e is enqueued once the records of iterations < e - ahead have been seen
        // (a sliding window: the device always has up to `ahead` iterations queued).  With
        // image shards (`reduce`) that window is exact -- the blocking wait ignores the lag
        // knob -- so a rank never has more than stop + 1 + ahead iterations enqueued, and
        // every rank is topped up to exactly that many below: the number of collectives is
        // the same on all ranks however late each host notices the stop (the surplus
        // iterations are launches that return at once around an all-reduce nobody reads).
        const bool shard = reduce != nullptr || comm_user != nullptr;   // image shards: collectives
        const int wlag = shard ? 0 : lag;
        if (persist_ok(p, c, vf, shard)) {
            // small problem: the first iteration as usual (it enters the single-array state),
            // every further one inside one launch
            enqueue_one();
            T *v0 = vb_in, *v1 = other_alt(v0);
            enq += run_persist(p, 1, c.max_iter, v0, v1, want_sums);
            if (c.need_residuals) poll(enq, false);
        }
        for (; enq < c.max_iter && stop_at < 0 && !persist_ok(p, c, vf, shard);) {
            enqueue_one();
            if (c.need_residuals) {
                poll(enq - lag, false);
                if (stop_at < 0 && enq - wlag - done > ahead) poll(enq - wlag - ahead, true);
            }
        }
        if (shard && want_sums && c.need_residuals) {
            if (stop_at < 0) poll(enq, true);       // (the last window: a stop may sit in it)
            if (stop_at >= 0)
                while (enq < c.max_iter && enq < stop_at + 1 + ahead) enqueue_one();
        }
        sync();
        poll(enq, false);
        const int n = stop_at >= 0 ? stop_at + 1 : enq;
        if (vf) {
            // iteration j wrote its V' to vr.out (j even) or to the other alt buffer (j odd);
            // thresholds as the control block formed them: (float)(lambda / rho of the iteration)
            auto held = [&](int j) {
                return held_v(p, (j & 1) ? other_alt(vr.out) : vr.out, (T)(p.lmbda / rec_ring[j].rho),
                              (T)(p.mu / rec_ring[j].rho));
            };
            const HeldV cur = held(n - 1), before = n >= 2 ? held(n - 2) : vr.in;
            commit_v(p, cur, before.buf ? &before : nullptr);
        } else {
            // launches enqueued after the stopping iteration did nothing: undo their buffer swaps --
            // and that of iteration n - 1, which commit_yu() makes
            if ((enq - n + 1) & 1) swap_alt_pair();
            commit_yu(p);
        }
        AdmmCtl fin;
        SA_HIP(hipMemcpy(&fin, ctl_dev, sizeof(AdmmCtl), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            const AdmmRecord &r = rec_ring[i];
            sporco_amd_admm_record &o = records[i];
            for (int j = 0; j < kOutSlots; ++j) o.sums[j] = r.sums[j];
            o.r = r.r;
            o.s = r.s;
            o.epri = r.epri;
            o.edua = r.edua;
            o.rho = r.rho;
            o.u_scale = r.u_scale;
            o.seconds = (double)r.ticks * 1e-8;
            o.k = r.k;
            o.stop = r.stop;
        }
        *rho_out = fin.rho;
        *u_scale_out = fin.u_scale;
        // host-side mirrors of the state the per-iteration path keeps
        stable_run = fin.stable_run > 0 ? fin.stable_run - 1 : 0;   // (admm_iter_fused re-derives it)
        if (fin.u_scale != 1.0) stable_run = 0;
        t_ready = fin.emitted != 0;
        last_p.rho = rec_ring[n - 1].rho;      // (the commit above took the rest from p)
        last_p.u_scale = rec_ring[n - 1].u_scale;
        return n;
    }

    // X = irfft_W(tile-major spectrum in the Xf buffer) / (H W): the row pass of
    // rows_inv_prox_fwd with a zero threshold (soft(v, 0) = v) and no forward half
    void rows_inverse_to(T *Xout, const cx<T> *t_in = nullptr) {
        auto ra = rows_prox_args();
        ra.t_in = t_in ? t_in : cv(SPORCO_AMD_VAR_XF);
        ra.Ks = t_in ? 0 : Ks;
        ra.t_out = nullptr;
        ra.x = Xout;
        ra.thr = T(0);
        ra.flags = 0;
        ra.dH = 1;
        ra.dW = 1;
        ProfScope ps(prof, PS_FFT_C2R);
        launch_rows_inv_prox_fwd<T>(st, ra);
    }
