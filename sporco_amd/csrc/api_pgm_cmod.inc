// api_pgm_cmod.inc -- the handle of pgm.cmod CnstrMOD / WeightedCnstrMOD (sporco/pgm/cmod.py:24-407); kernels:
// csc_pgm_cmod.h.  Included by csc_api.hip at namespace scope, after api_cmod.inc: the handle is Cmod<T> with the
// arrays of the proximal gradient iteration added, so S and Z (own copies or device pointers read in place), the
// k-major uploads and downloads, cmod_dfid, the stream and the profile slots are that handle's.  Its arrays xk / uk
// serve as the two X arrays (the iterate and the one before it; a step may start by swapping their roles), yk / bk as
// the two Y arrays, sztk as G.  One table of partial sums, a row per workgroup and a column per sum, serves every
// kernel of a step: a kernel writes its own columns of its own rows, the rows beyond stay zero, and one reduction
// launch reads the table.
template <typename T> struct PgmCmod : Cmod<T> {
    using B = Cmod<T>;
    const PgmCmodPlan pp;
    int cx = 0, cy = 0;            // which X array holds the iterate, which Y array the Y in use
    T *zv = nullptr, *zz = nullptr, *part_pg = nullptr, *w_own = nullptr;
    const T *w = nullptr;
    T w_s = T(1);                  // the scalar weight of the last step (read where w is null)
    double *table = nullptr;
    int rows = 1;

    PgmCmod(int N_, int M_, int64_t K_, int dev, void *stream)
        : B(N_, M_, K_, dev, stream), pp(pgm_cmod_plan(N_, M_, K_)) {
        rows = pp.NRB * pp.nsplit;
        rows = std::max(rows, pgm_cmod_reduce_blocks(this->M, pp.N16));
        rows = std::max(rows, std::max(this->nb_dfid, this->nb_iter));
        table = this->template dev_alloc<double>((size_t)kPgmCmodSums * rows, true);
        part_pg = this->template dev_alloc<T>((size_t)pp.nsplit * pp.M16 * pp.N16, false);
        for (T **p : {&zv, &zz}) *p = this->template dev_alloc<T>(this->kmaj(), true);
        this->sync();
    }

    void plan(int64_t out[8]) override {
        out[0] = kCmodKS;
        out[1] = pp.slab;
        out[2] = pp.nsplit;
        out[3] = pp.NRB;
        out[4] = pp.ctw;
        out[5] = this->form;
        out[6] = (int64_t)pgm_cmod_grad_lds_bytes<T>(this->M);
        out[7] = (int64_t)pgm_cmod_prox_lds_bytes<T>(this->N);
    }
    // (no Gram matrices: the weight sits between the two products)
    void set_coef(const void *Z, bool on_device) override { this->take(Z, on_device, this->M, &this->z_own, &this->z); }
    void set_weight(const void *W, bool on_device) override {
        if (!W) {
            this->sync();
            w = nullptr;
            return;
        }
        this->take(W, on_device, this->N, &w_own, &w);
    }
    void set_solve(const void *) override { throw Error(SPORCO_AMD_EINVAL, "cmod: a pgm handle has no solve matrix"); }
    void iter(const sporco_amd_cmod_params &, double *) override {
        throw Error(SPORCO_AMD_EINVAL, "cmod: a pgm handle steps by sporco_amd_cmod_pgm_step");
    }

    T *xbuf(int which) { return which == 0 ? this->xk : this->uk; }
    T *ybuf(int which) { return which == 0 ? this->yk : this->bk; }
    T *kbuf(int var) override {
        switch (var) {
        case SPORCO_AMD_CMOD_X: return xbuf(cx);
        case SPORCO_AMD_CMOD_XPRV: return xbuf(cx ^ 1);
        case SPORCO_AMD_CMOD_Y: return ybuf(cy);
        case SPORCO_AMD_CMOD_YALT: return ybuf(cy ^ 1);
        case SPORCO_AMD_CMOD_PG: return this->sztk;
        case SPORCO_AMD_CMOD_PZ: return zv;
        case SPORCO_AMD_CMOD_ZZ: return zz;
        default: throw Error(SPORCO_AMD_EINVAL, "cmod: unknown array id");
        }
    }

    void launch_dfid_w(const T *fk, bool gz2, T ws) {
        CmodDfidArgs<T> d;
        d.fk = fk;
        d.z = this->z;
        d.s = gz2 ? nullptr : this->s;
        d.w = gz2 ? nullptr : w;
        d.w_s = gz2 ? T(1) : ws;
        d.M = this->M;
        d.N = this->N;
        d.K = this->K;
        d.KB = this->KB;
        d.form = this->form;
        d.partials = table + (gz2 ? PGMC_GZ2 : PGMC_FX);
        d.stride = kPgmCmodSums;
        ProfScope ps(this->prof, PS_CMOD_PGM_DFID);
        launch_cmod_dfid<T>(this->st, d);
    }

    void finalize(double *out_host) {
        // (pgm_cmod_sums order = the SPORCO_AMD_PGMC_* slots; the halves of f) in two groups of the one reduction launch
        const int slots[8] = {0, 1, 2, 3, 4, 5, 6, 7}, slots_b[3] = {8, 9, 10};
        const double scales[8] = {0.5, 0.5, 1, 1, 1, 1, 1, 1}, ones[3] = {1, 1, 1};
        {
            ProfScope ps(this->prof, PS_FINALIZE);
            launch_finalize2(this->st, table, rows, kPgmCmodSums, 8, slots, scales, table + 8, rows, kPgmCmodSums, 3, slots_b,
                             ones, this->out_dev);
        }
        if (out_host) this->read_out(out_host);
    }

    void pgm_step(const sporco_amd_cmod_pgm_params &p, double *out_host) override {
        SA_REQUIRE(this->s && this->z, "cmod: S and the coefficients are set before the first step");
        SA_REQUIRE(p.L > 0.0, "L must be positive");
        const int known = SPORCO_AMD_PGMC_PHASE_YROBUST | SPORCO_AMD_PGMC_PHASE_GRAD | SPORCO_AMD_PGMC_PHASE_GZ2 |
                          SPORCO_AMD_PGMC_PHASE_PROX | SPORCO_AMD_PGMC_PHASE_DFID;
        SA_REQUIRE((p.phase & ~known) == 0, "cmod: unknown phase");
        if (p.advance) cx ^= 1;
        if (p.advance_y) cy ^= 1;
        w_s = (T)p.w;
        if (p.phase & SPORCO_AMD_PGMC_PHASE_YROBUST) {
            ProfScope ps(this->prof, PS_CMOD_PGM_YROBUST);
            launch_cmod_pgm_yrobust<T>(this->st, xbuf(cx ^ 1), ybuf(cy ^ 1), zv, ybuf(cy), (T)p.tk, (T)p.t, (T)(p.tk + p.t),
                                       (T)p.zc, p.z_update, (int)this->kmaj());
        }
        if (p.phase & SPORCO_AMD_PGMC_PHASE_GRAD) {
            PgmCmodGradArgs<T> a;
            a.z = this->z;
            a.s = this->s;
            a.w = w;
            a.w_s = w_s;
            a.yk = ybuf(cy);
            a.part = part_pg;
            a.gk = this->sztk;
            a.xprvk = xbuf(cx ^ 1);
            a.xoldk = xbuf(cx);
            a.bb = p.bb;
            a.form = this->form;
            a.M = this->M;
            a.N = this->N;
            a.K = this->K;
            a.p = pp;
            a.partials = table;
            {
                ProfScope ps(this->prof, PS_CMOD_PGM_GRAD);
                launch_cmod_pgm_grad<T>(this->st, a);
            }
            {
                ProfScope ps(this->prof, PS_CMOD_PGM_REDUCE);
                launch_cmod_pgm_reduce<T>(this->st, a);
            }
        }
        if (p.phase & SPORCO_AMD_PGMC_PHASE_GZ2) launch_dfid_w(this->sztk, true, T(1));
        if (p.phase & SPORCO_AMD_PGMC_PHASE_PROX) {
            PgmCmodProxArgs<T> a;
            a.yk = ybuf(cy);
            a.gk = this->sztk;
            a.xprvk = xbuf(cx ^ 1);
            a.yprvk = p.yprv_alt ? ybuf(cy ^ 1) : nullptr;
            a.zzk_in = zz;
            a.xk = xbuf(cx);
            a.ynextk = p.write_y ? ybuf(cy ^ 1) : nullptr;
            a.zzk = p.keep_zz ? zz : nullptr;
            a.L = (T)p.L;
            a.beta = (T)p.beta;
            a.gamma = (T)p.gamma;
            a.zero_mean = p.zero_mean;
            a.nonneg = p.nonneg;
            a.revert = p.revert;
            a.rs_ynext = p.rs_ynext;
            a.M = this->M;
            a.N = this->N;
            a.partials = table;
            SA_REQUIRE(!(p.yprv_alt && p.write_y), "cmod: the other Y array is read or written, not both");
            ProfScope ps(this->prof, PS_CMOD_PGM_PROX);
            launch_cmod_pgm_prox<T>(this->st, a);
        }
        if (p.phase & SPORCO_AMD_PGMC_PHASE_DFID) launch_dfid_w(xbuf(cx), false, w_s);
        if (p.finalize) finalize(out_host);
    }

    // sum w (X Z - S)^2 of the iterate with the Z, S and weight array in use (the half and a scalar weight are the caller's)
    void dfid(int var, double *out_host) override {
        SA_REQUIRE(this->s && this->z, "cmod: S and the coefficients are set first");
        SA_REQUIRE(var == SPORCO_AMD_CMOD_X, "cmod: a pgm handle takes DFid at X");
        launch_dfid_w(xbuf(cx), false, T(1));
        const int slots_d[1] = {SPORCO_AMD_OUT_DFID};
        const double ones[1] = {1};
        {
            ProfScope ps(this->prof, PS_FINALIZE);
            launch_finalize(this->st, table + PGMC_FX, rows, kPgmCmodSums, 1, slots_d, ones, false, this->out_dev);
        }
        this->read_out(out_host);
    }
};

CmodBase *make_pgm_cmod(int dtype, int N, int M, int64_t K, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new PgmCmod<float>(N, M, K, device, stream);
    if (dtype == SPORCO_AMD_F64) return new PgmCmod<double>(N, M, K, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
