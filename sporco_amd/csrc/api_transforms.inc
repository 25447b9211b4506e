// api_transforms.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): generic 2-D transforms, tile-major operands of the fused X-step, single-array (V) state.
    // ---- 2-D transforms with per-kernel timing -------------------------------
    // the transform along the (folded) first axis of an array (H, Wf, cols): one pass -- or, on a
    // volume handle, along the height inside every depth slab and then along the depth
    void c2c_first_axis(bool inverse, const cx<T> *in, cx<T> *out, int64_t cols) {
        const int64_t line = (int64_t)Wf * cols, slab = (int64_t)Hs * line;
        fft_c2c<T>(st, planH, inverse, in, out, depth, line, slab, line, slab, line, T(1));
        if (depth > 1) fft_c2c<T>(st, planD, inverse, out, out, 1, slab, 0, slab, 0, slab, T(1));
    }
    void fwd2(const T *in, const T *in2, T s2, cx<T> *out, int64_t cols,
              const VformIn<T> *vf = nullptr) {
        {
            ProfScope ps(prof, PS_FFT_R2C);
            fft_r2c<T>(st, planW, in, in2, s2, out, H, cols, (int64_t)W * cols, cols,
                       (int64_t)Wf * cols, cols, 0, 0, 0, vf);
        }
        {
            ProfScope ps(prof, PS_FFT_C2C_FWD);
            c2c_first_axis(false, out, out, cols);
        }
    }
    // The generic chain's fused row pass (fft.h fft_c2r_vpost): X never leaves the kernel; while
    // md_x_pending with gx_buf set, X is one c2r row pass of that buffer away (materialize_x).  The
    // emitted row spectrum goes to `gemit` and the two buffers trade places, so the column pass's
    // output stays intact until the next one.
    cx<T> *gemit = nullptr, *gx_buf = nullptr;
    double *part_vpost = nullptr;
    int64_t part_vpost_cap = 0;
    void inv2(const cx<T> *in, cx<T> *tmp, T *out, int64_t cols) {
        {
            ProfScope ps(prof, PS_FFT_C2C_INV);
            c2c_first_axis(true, in, tmp, cols);
        }
        {
            ProfScope ps(prof, PS_FFT_C2R);
            fft_c2r<T>(st, planW, tmp, out, H, cols, (int64_t)Wf * cols, cols, (int64_t)W * cols,
                       cols, T(1.0 / ((double)H * (double)W)));
        }
    }

    // The column pass for 64 < K <= 256: one launch of cooperating slab workgroups.  Returns the
    // number of tiles.
    int64_t run_slab_cols(FusedSlabArgs<T> &sa) {
        coop_prepare(sa);
        return launch_cols_slab_coop<T>(st, sa);
    }
    // flags, launch counter and error word of a launch of cooperating slab workgroups
    void coop_prepare(FusedSlabArgs<T> &sa) {
        if (!coop_flags) {
            const size_t n = sizeof(unsigned) * (size_t)Wf * CN * ((K + 63) / 64);
            SA_HIP(hipMalloc((void **)&coop_flags, n));
            SA_HIP(hipMemsetAsync(coop_flags, 0, n, st));
            SA_HIP(hipHostMalloc((void **)&coop_err, sizeof(int), 0));
            *coop_err = 0;
        }
        sa.coop_flags = coop_flags;
        sa.coop_seq = ++coop_seq;
        sa.coop_err = coop_err;
    }

    void finalize(const double *part, int nblocks, int stride, int nvals, const int *slots,
                  const double *scales, double *out_dev, bool is_max = false) {
        ProfScope ps(prof, PS_FINALIZE);
        launch_finalize(st, part, nblocks, stride, nvals, slots, scales, is_max, out_dev);
    }

    // ---- the sum tables of the ADMM iterations ------------------------------------------------
    // An epilogue (launch_admm_post, the row epilogues, admm_stats) leaves rows of 8 partials; their
    // first nvals columns go to these slots.  with_s2 false: the dual residual is summed elsewhere
    // (the two-block classes) and S2 stays at zero.
    static constexpr int kPostSlots[7] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_AX2,
                                          SPORCO_AMD_OUT_Y2, SPORCO_AMD_OUT_U2, SPORCO_AMD_OUT_L1,
                                          SPORCO_AMD_OUT_L21};
    static constexpr double kPostScales[2][7] = {{1, 0, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1}};
    void finalize_post(const double *part, int nb, int nvals, bool with_s2, double *out_dev) {
        finalize(part, nb, 8, nvals, kPostSlots, kPostScales[with_s2 ? 1 : 0], out_dev);
    }
    // A solve leaves rows of nvals partials in part_a: the data fidelity (dfid_scale 0: the solve
    // ran against a block-0 spectrum and its residual is no statistic), the LinSolveCheck triple
    // and, nvals = 5, the gradient term, which goes to grad_slot (OUT_RGR or OUT_RGRX)
    void finalize_solve(int nb, int nvals, double dfid_scale, int grad_slot, double *out_dev) {
        const int slots[5] = {SPORCO_AMD_OUT_DFID, SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2,
                              SPORCO_AMD_OUT_XRRS_B2, grad_slot};
        const double scales[5] = {dfid_scale, 1.0, 1.0, 1.0, 1.0 / ((double)H * W)};
        finalize(part_a, nb, nvals, nvals, slots, scales, out_dev);
    }

    // the sums of a three-launch iteration in one launch over both partial arrays: the six (joint:
    // seven) of the `nt` row tiles of the epilogue, and the column kernel's data-fidelity (and
    // gradient) term
    void finalize_iter_sums(const sporco_amd_admm_params &p, int64_t nt, double *out_dev) {
        const int *slots = kPostSlots;
        const double *scales = kPostScales[1];
        const int nrow = (p.flags & F_JOINT) ? 7 : 6;
        const int fslots[2] = {SPORCO_AMD_OUT_DFID, SPORCO_AMD_OUT_RGR};
        const double fscales[2] = {1.0 / ((double)H * W), 1.0 / ((double)H * W)};
        const bool dfid = (p.flags & F_OBJ) && !(p.flags & F_FEVAL_Y);
        const int fnv = (p.flags & F_GRADREG) ? 2 : 1;
        ProfScope ps(prof, PS_FINALIZE);
        launch_finalize2(st, part_rows, (int)nt, 8, nrow, slots, scales, part_f, part_f_rows, fnv,
                         dfid ? fnv : 0, fslots, fscales, out_dev);
    }

    // ---- argument structs of the register-resident passes -------------------------------------
    // Each builder sets every field that is the same wherever this handle launches the pass; a call
    // site adds what is its own (the routing of the iterate, thresholds, ctl, tail / gradient extras).
    // rows_fwd into the Xf buffer (rows Ks filters apart) or into `t` (rows of K filters)
    RowsFwdArgs<T> rows_fwd_args(cx<T> *t = nullptr) {
        RowsFwdArgs<T> ra;
        ra.y = ra.u = nullptr;
        ra.t = t ? t : cv(SPORCO_AMD_VAR_XF);
        ra.Ks = t ? 0 : Ks;
        ra.twA = twRows;
        ra.H = H;
        ra.W = W;
        ra.C = C;
        ra.N = N;
        ra.CN = CN;
        ra.K = K;
        ra.P = P;
        return ra;
    }
    // ... of an iterate held as V, with what the derivation of (Y, U) repeats: thresholds from the
    // iterate, options from p -- the parameters of the iteration that reads it (the same options
    // as the iterate's own: enter_iteration)
    RowsFwdArgs<T> rows_fwd_args(const HeldV &v, const sporco_amd_admm_params &p, cx<T> *t = nullptr) {
        RowsFwdArgs<T> ra = rows_fwd_args(t);
        ra.v = v.buf;
        ra.thr_prev = v.thr;
        ra.thr21_prev = v.thr21;
        ra.flags = p.flags;
        ra.wl1 = wl1;
        ra.dH = p.dH;
        ra.dW = p.dW;
        ra.ams_bits = ams_bits_of(p);
        ra.ams_k = Ku - 1;
        return ra;
    }
    void run_rows_fwd(const RowsFwdArgs<T> &ra) {
        ProfScope ps(prof, ra.v ? PS_ROWS_FWD_V : PS_ROWS_FWD);
        launch_rows_fwd<T>(st, ra);
    }
    void launch_rows_fwd_on(const T *Yin, const T *Uin, T s2) {
        auto ra = rows_fwd_args();
        ra.y = Yin;
        ra.u = Uin;
        ra.s2 = s2;
        run_rows_fwd(ra);
    }
    // the column pass on the Xf buffer (or `t`) with the handle's dictionary and signal (striped: its
    // output goes to cols_out[], csc_fused.h)
    FusedColsArgs<T> fused_cols_args(double rho, bool striped = false, cx<T> *t = nullptr) {
        FusedColsArgs<T> fa;
        fa.t = t ? t : cv(SPORCO_AMD_VAR_XF);
        fa.dft = dft;
        fa.sft = sft;
        fa.gramt = gramt;
        fa.twA = twA;
        fa.twB = twB;
        fa.rho = (T)rho;
        fa.H = H;
        fa.W = W;
        fa.CN = CN;
        fa.K = K;
        fa.partials = part_f;
        fa.Ks = Ks;
        if (striped) {
            fa.out_even = cols_out[0];
            fa.out_odd = cols_out[1];
        }
        return fa;
    }
    // the row epilogue reading the Xf buffer (striped: cols_out[]); no iterate routed, nothing
    // emitted, no X: the call site sets those, thr / thr21 / u_scale and, where it has one, ctl
    RowsPostArgs<T> rows_post_args(const sporco_amd_admm_params &p, bool striped = false) {
        RowsPostArgs<T> pa;
        pa.t = cv(SPORCO_AMD_VAR_XF);
        if (striped) {
            pa.t = cols_out[0];
            pa.t_odd = cols_out[1];
        }
        pa.twW = planW.tw<T>();
        pa.twA = twRows;
        pa.t_next = nullptr;
        pa.y = pa.u = nullptr;
        pa.y_out = pa.u_out = nullptr;
        pa.x = nullptr;
        pa.scale = T(1.0 / ((double)H * (double)W));
        pa.rlx = (T)p.rlx;
        pa.flags = p.flags;
        pa.H = H;
        pa.W = W;
        pa.C = C;
        pa.N = N;
        pa.K = K;
        pa.dH = p.dH;
        pa.dW = p.dW;
        pa.P = P;
        pa.wl1 = wl1;
        pa.Ks = Ks;
        pa.ams_bits = ams_bits_of(p);
        pa.ams_k = Ku - 1;
        pa.partials = part_rows;
        return pa;
    }
    // the inverse row pass with a prox (FISTA; X on demand): transforms, dimensions, partials
    RowsProxArgs<T> rows_prox_args() {
        RowsProxArgs<T> ra;
        ra.twA = twRows;
        ra.twW = planW.tw<T>();
        ra.scale = T(1.0 / ((double)H * (double)W));
        ra.H = H;
        ra.W = W;
        ra.C = C;
        ra.N = N;
        ra.K = K;
        ra.P = P;
        ra.partials = part_rows;
        return ra;
    }
    // the streaming epilogue (launch_admm_post, fft_c2r_vpost) on the (Y, U) form of x, y, u with the
    // plain l1 threshold: the call site adds the routing of a single-array iterate (v_in / v_out /
    // thr_prev), thr21 under F_JOINT and dy_out.  The AddMaskSim fields are read under F_AMS only.
    PostParams<T> post_params(const sporco_amd_admm_params &p, const T *x, T *y, T *u) {
        PostParams<T> pp;
        pp.x = x;
        pp.y = y;
        pp.u = u;
        pp.rlx = (T)p.rlx;
        pp.thr = (T)(p.lmbda / p.rho);
        pp.thr21 = T(0);
        pp.u_scale = (T)p.u_scale;
        pp.flags = p.flags;
        pp.d = d5();
        pp.dH = p.dH;
        pp.dW = p.dW;
        pp.wl1 = wl1;
        pp.wl21 = wl21;
        pp.ams = ams_of(p);
        pp.ams_k = ams_k0();
        pp.ams_n = ams_n();
        return pp;
    }

    // ---- tile-major operands of the fused X-step -----------------------------------
    void refresh_fused_dict() {
        if (fused_mc) {
            ProfScope ps(prof, PS_OTHER);
            launch_permute_ab<cx<T>>(st, cv(SPORCO_AMD_VAR_DF), dft_mc, H, Wf, (int64_t)Cd * K);
            binv_valid = false;
            return;
        }
        if (!fused && !fused_slabs) return;
        ProfScope ps(prof, PS_OTHER);
        launch_permute_ab<cx<T>>(st, cv(SPORCO_AMD_VAR_DF), dft, H, Wf, K, 0, Ks);
        launch_permute_ab<T>(st, gram, gramt, H, Wf, 1);
        g1_valid = false;
    }
    void refresh_fused_signal() {
        if (fused_mc) {
            ProfScope ps(prof, PS_OTHER);
            launch_permute_ab<cx<T>>(st, cv(SPORCO_AMD_VAR_SF), sft_mc, H, Wf, (int64_t)CNs);
            return;
        }
        if (!fused && !fused_slabs) return;
        ProfScope ps(prof, PS_OTHER);
        launch_permute_ab<cx<T>>(st, cv(SPORCO_AMD_VAR_SF), sft, H, (int64_t)Wf * CN, 1);
    }
    // ---- single-array state (csc_rows.h): back to the (Y, U) form ----------------------------
    bool vform_ok(const sporco_amd_admm_params &p) const {
        return !sw.no_vform && std::is_same<T, float>::value && rows_ok && mr_ok(p) &&
               !(p.flags & (F_KEEP_X | F_FEVAL_Y | F_XRRS)) &&
               (!(p.flags & F_JOINT) || joint_rows_ok(p));
    }
    // the held V was produced under the options of p (otherwise: back to (Y, U) first)
    static bool vform_same_opts(const HeldV &v, const sporco_amd_admm_params &p) {
        const uint32_t o = p.flags & (F_NOBNDRY | F_AMS);
        return (bool)(p.flags & F_NONNEG) == v.nonneg && (bool)(p.flags & F_JOINT) == v.joint &&
               o == v.opts && (!(o & F_NOBNDRY) || (p.dH == v.dH && p.dW == v.dW));
    }
    // an iterate that an iteration with the parameters p leaves (or left) as V in `buf`
    static HeldV held_v(const sporco_amd_admm_params &p, T *buf, T thr, T thr21) {
        HeldV v;
        v.buf = buf;
        v.thr = thr;
        v.thr21 = thr21;
        v.nonneg = p.flags & F_NONNEG;
        v.joint = p.flags & F_JOINT;
        v.opts = p.flags & (F_NOBNDRY | F_AMS);
        v.dH = p.dH;
        v.dW = p.dW;
        return v;
    }
    // Y (and / or U) of an iterate held as V: y or u may be null, u may alias v.buf
    void vform_split(const HeldV &v, T *y, T *u) {
        if (v.joint)
            launch_vform_split_joint<T>(st, v.buf, y, u, v.thr, v.thr21, v.nonneg, C, (int64_t)N * K,
                                        (int64_t)H * W);
        else if (wl1.ptr || v.opts)
            launch_vform_split_general<T>(st, v.buf, y, u, v.thr,
                                          (v.nonneg ? F_NONNEG : 0u) | (v.opts & F_NOBNDRY), d5(),
                                          v.dH, v.dW, wl1, (v.opts & F_AMS) ? wams : Weight<T>(),
                                          Ku - 1);
        else
            launch_vform_split<T>(st, v.buf, y, u, v.thr, v.nonneg, E);
    }
    // the generic chain keeps the single array too (admm_iter): plain l1 term, no option that
    // needs the 5-D index of an element or Y itself, and an X-step that reads (Y, U) through the
    // generic row transform
    bool gvform_ok(const sporco_amd_admm_params &p) const {
        return !sw.no_vform && !wl1.ptr &&
               !(p.flags & (F_JOINT | F_NOBNDRY | F_AMS | F_FEVAL_Y | F_XRRS)) &&
               !(rows_ok && (fused || fused_slabs || fused_mc));
    }
    T *other_alt(const T *b) const { return b == y_alt ? u_alt : y_alt; }
    void swap_alt_pair() {
        std::swap(vars[SPORCO_AMD_VAR_Y], reinterpret_cast<void *&>(y_alt));
        std::swap(vars[SPORCO_AMD_VAR_U], reinterpret_cast<void *&>(u_alt));
    }
    // ---- transitions of the iterate record (csc_api.hip `it`) ---------------------------------
    // Entry of a fused iteration or run with the parameters p.  A held V that p cannot continue goes
    // back to (Y, U); `in` is the V the first iteration reads (buf null: it reads (Y, U) from vars),
    // `out` the buffer its V' goes to (null: the (Y, U) form).  A live V is always continued; want_v
    // says whether the caller enters the V form from (Y, U).  The alt pair must exist by now.
    struct VRoute {
        HeldV in;
        T *out = nullptr;
    };
    VRoute enter_iteration(const sporco_amd_admm_params &p, bool want_v) {
        if (it.form == IterForm::GenericV) ensure_yu();
        if (it.form == IterForm::FusedV && !(vform_ok(p) && vform_same_opts(it.cur, p))) ensure_yu();
        VRoute r;
        const bool live = it.form == IterForm::FusedV;
        if (!live && !(want_v && vform_ok(p))) return r;
        if (live) r.in = it.cur;
        r.out = other_alt(r.in.buf);
        return r;
    }
    // what both forms of a fused iteration leave behind: X exists on demand (materialize_x, from the
    // previous iterate and last_p)
    void commit_common(const sporco_amd_admm_params &p) {
        last_p = p;
        x_stale = true;
        x_invalid = p.flags & F_NO_X;
    }
    // ... in the V form: `cur` is the new iterate, `prev` the V before it (in the other alt buffer),
    // or null when the previous iterate is the (Y, U) in vars that the only iteration read
    void commit_v(const sporco_amd_admm_params &p, const HeldV &cur, const HeldV *prev) {
        if (prev) it.prev = *prev;
        it.prev_at = prev ? PrevAt::AltV : PrevAt::VarsYU;
        it.cur = cur;
        it.form = IterForm::FusedV;
        commit_common(p);
    }
    // ... in the (Y, U) form: the new iterate went to (y_alt, u_alt) and the pairs swap roles
    void commit_yu(const sporco_amd_admm_params &p) {
        swap_alt_pair();
        it.prev_at = PrevAt::AltYU;
        commit_common(p);
    }
    void ensure_yu() {
        if (it.form == IterForm::YU) return;
        const bool generic = it.form == IterForm::GenericV;
        it.form = IterForm::YU;
        ProfScope ps(prof, PS_OTHER);
        T *const Yv = static_cast<T *>(vars[SPORCO_AMD_VAR_Y]), *const Uv = static_cast<T *>(vars[SPORCO_AMD_VAR_U]);
        HeldV cur = it.cur;
        if (generic) {     // in place: V lives in the buffer of U
            cur.buf = Uv;
            vform_split(cur, Yv, Uv);
            return;
        }
        T *other = other_alt(cur.buf);
        if (it.prev_at == PrevAt::VarsYU) {
            // vars hold the previous iterate as (Y, U) and the other alt buffer is free: the
            // new pair goes to (other, cur.buf) and the buffers trade places -- exactly the state
            // an iteration of the (Y, U) form leaves behind
            vform_split(cur, other, cur.buf);
            vars[SPORCO_AMD_VAR_Y] = other;
            vars[SPORCO_AMD_VAR_U] = cur.buf;
            y_alt = Yv;
            u_alt = Uv;
            it.prev_at = PrevAt::AltYU;
        } else {
            vform_split(cur, Yv, Uv);
            // the previous iterate (it.prev, in `other`) stays in V form until somebody asks for it
            it.prev_at = it.prev_at == PrevAt::AltV ? PrevAt::PendingV : PrevAt::None;
            it.prev_free = cur.buf;
        }
    }
    void ensure_prev_yu() {
        ensure_yu();
        if (it.prev_at != PrevAt::PendingV) return;
        ProfScope ps(prof, PS_OTHER);
        vform_split(it.prev, it.prev_free, it.prev.buf);
        y_alt = it.prev_free;
        u_alt = it.prev.buf;
        it.prev_at = PrevAt::AltYU;
    }

    // X of the last three-launch iteration, rebuilt from the previous iterate.
    void materialize_x() {
        if (x_invalid)
            throw Error(SPORCO_AMD_ESTATE,
                        "X / Xf of an iteration run with SPORCO_AMD_FLAG_NO_X were requested");
        if (pgm_x_stale) {
            pgm_x_stale = false;
            pgm_rows_prox(last_pgm, work_buf(), nullptr, rv(SPORCO_AMD_VAR_X), nullptr);
        }
        if (md_x_pending && gx_buf) {
            // the generic chain's fused row pass: the column pass's output (natural layout) waits
            // in gx_buf
            md_x_pending = false;
            ProfScope ps(prof, PS_FFT_C2R);
            fft_c2r<T>(st, planW, gx_buf, rv(SPORCO_AMD_VAR_X), H, P, (int64_t)Wf * P, P, (int64_t)W * P, P,
                       T(1.0 / ((double)H * (double)W)));
            gx_buf = nullptr;
        }
        if (md_x_pending) {
            // the fused mask-decoupled iteration (api_maskdcpl.inc) left the column-inverse-
            // transformed solution in the Xf buffer: X is one row pass away
            md_x_pending = false;
            rows_inverse_to(rv(SPORCO_AMD_VAR_X));
        }
        if (!x_stale) return;
        ensure_prev_yu();
        x_stale = false;
        t_ready = false;   // the Xf buffer is about to be reused
        sporco_amd_admm_params q = last_p;
        q.flags = last_p.flags & F_GRADREG;   // (the system solved, not the sums wanted)
        launch_rows_fwd_on(y_alt, u_alt, (T)q.u_scale);
        run_fused_cols(q, nullptr);
        rows_inverse_to(rv(SPORCO_AMD_VAR_X));
    }
    // call before reading `var` / before changing anything X depends on
    void before_read(int var) {
        ++touch_epoch;
        if (var == SPORCO_AMD_VAR_X || var == SPORCO_AMD_VAR_XF) materialize_x();
        need_natural(var);
    }
    void before_state_change() {
        ++touch_epoch;
        pgm_rx_count = 0;
        if ((x_stale && !x_invalid) || pgm_x_stale || md_x_pending) materialize_x();
        ensure_yu();
        it.prev_at = PrevAt::None;
        t_ready = false;
    }
    // The dictionary changes: a pending X depends on the old one, but the speculatively emitted
    // row spectra of Y - U (t_ready) and the ping-pong parity do not -- a dictionary-learning
    // loop keeps skipping the forward row pass of its one-iteration X-steps.
    void before_dict_change() {
        ++touch_epoch;
        pgm_rx_count = 0;
        if ((x_stale && !x_invalid) || pgm_x_stale || md_x_pending) materialize_x();
    }
    void x_written() {
        x_stale = false;
        x_invalid = false;
        pgm_x_stale = false;
        md_x_pending = false;
        gx_buf = nullptr;
    }
    static bool is_pgm_iterate(int var) {
        return var == SPORCO_AMD_VAR_XF || var == SPORCO_AMD_VAR_YF ||
               var == SPORCO_AMD_VAR_XFPRV || var == SPORCO_AMD_VAR_YFPRV;
    }
    // The scratch spectra of the host-composed policies (VAR_T0..T2: Z of robust backtracking, ZZ
    // of monotone FISTA) follow the iterates into the tile-major layout when they are combined
    // with them there (lincomb / pair_stats below), each on its own flag; any other access takes
    // the one it touches back to the reference layout.
    bool aux_tiled[3] = {false, false, false};
    static int aux_slot(int var) {
        return (var >= SPORCO_AMD_VAR_T0 && var <= SPORCO_AMD_VAR_T2) ? var - SPORCO_AMD_VAR_T0 : -1;
    }
    void aux_written_natural(int var) {
        if (aux_slot(var) >= 0) aux_tiled[aux_slot(var)] = false;
    }
    // every variable of the call is an iterate or a scratch spectrum, and the iterates are tile-major
    bool tiled_operands(std::initializer_list<int> vs) const {
        if (!pgm_tiled || Ks != K) return false;
        for (int v : vs)
            if (v >= 0 && !is_pgm_iterate(v) && aux_slot(v) < 0) return false;
        return true;
    }
    void aux_to_tiled(int var) {
        const int s = aux_slot(var);
        if (s < 0 || aux_tiled[s]) return;
        (void)cv(var);
        relayout(var, true);
        aux_tiled[s] = true;
    }
    // natural (H, Wf*CN, K) <-> tile-major (Wf*CN, H, K) of one X-sized spectrum, through
    // the column-pass scratch buffer (pointer swap, no second copy)
    void relayout(int var, bool to_tiled) {
        cx<T> *src = cv(var), *dst = work_buf();
        const int64_t ks = var == SPORCO_AMD_VAR_XF ? Ks : K;   // row stride of the tiled side
        {
            ProfScope ps(prof, PS_OTHER);
            if (to_tiled)
                launch_permute_ab<cx<T>>(st, src, dst, H, (int64_t)Wf * CN, K, K, ks);
            else
                launch_permute_ab<cx<T>>(st, src, dst, (int64_t)Wf * CN, H, K, ks, K);
        }
        vars[var] = dst;
        work = src;
    }
    void pgm_leave_tiled() {
        pgm_rx_count = 0;      // (the masked iteration's residual history follows the tiled iterates)
        if (!pgm_tiled) return;
        if (pgm_x_stale) materialize_x();   // needs `work` before it is reused as scratch
        pgm_tiled = false;
        for (int v : {SPORCO_AMD_VAR_XF, SPORCO_AMD_VAR_YF, SPORCO_AMD_VAR_XFPRV,
                      SPORCO_AMD_VAR_YFPRV})
            relayout(v, false);
    }

    // VAR_XF as callers know it (natural layout): after a fused X-step the buffer
    // holds a tile-major intermediate, and Xf = rfftn(X) is rebuilt on demand.
    void need_natural(int var) {
        if (var == SPORCO_AMD_VAR_XF) t_ready = false;
        if (aux_slot(var) >= 0 && aux_tiled[aux_slot(var)]) {
            if (pgm_x_stale) materialize_x();   // `work` is about to be used as scratch
            aux_tiled[aux_slot(var)] = false;
            relayout(var, false);
        }
        if (pgm_tiled && is_pgm_iterate(var)) pgm_leave_tiled();
        if (var == SPORCO_AMD_VAR_ZF && zf_tiled) {
            if (pgm_x_stale) materialize_x();   // `work` is about to be used as scratch
            zf_tiled = false;
            relayout(SPORCO_AMD_VAR_ZF, false);
        }
        if (var == SPORCO_AMD_VAR_XF && xf_tiled) {
            xf_tiled = false;
            fwd2(rv(SPORCO_AMD_VAR_X), nullptr, T(0), cv(SPORCO_AMD_VAR_XF), P);
        }
    }
