// api_rpca.inc -- the handle of RobustPCA (sporco/admm/rpca.py:23-262) and of the stateless prox_nuclear /
// norm_nuclear; kernels: csc_rpca.h.  It is included by csc_api.hip at namespace scope and keeps its stream, sums and buffers
// through SideBase (csc_impl.h).  S, X, Y, U
// are (R, C), row-major as NumPy has them, and stay so on the device: S either the handle's own copy of a host array
// or a device pointer read in place.  The Gram matrix goes to the host in double; T = W diag(f) W^T comes back in
// double and is laid out zero padded, [n4][n16], in the handle's precision (T is symmetric: that is k-major).
template <typename T> struct Rpca : RpcaBase {
    const int R, C;
    const RpcaPlan pl;
    int form_gram, form_iter;       // BPDN_FORM_MFMA on the device unless SPORCO_AMD_RPCA_PLAIN is set (iter: float32 only)
    T *s_own = nullptr;
    const T *s = nullptr;
    T *x = nullptr, *y = nullptr, *u = nullptr, *tk = nullptr;
    double *part_g = nullptr, *g = nullptr, *part = nullptr, *part_s = nullptr;
    std::vector<T> stage;

    size_t count() const { return (size_t)R * C; }
    size_t tk_count() const { return (size_t)pl.n4 * pl.n16; }

    Rpca(int R_, int C_, int dev, void *stream) : RpcaBase(dev, stream), R(R_), C(C_), pl(rpca_plan<T>(R_, C_)) {
#ifdef SPORCO_AMD_HOSTSIM
        form_gram = form_iter = BPDN_FORM_PLAIN;
#else
        const bool plain = Switches::set("SPORCO_AMD_RPCA_PLAIN");
        form_gram = plain ? BPDN_FORM_PLAIN : BPDN_FORM_MFMA;
        form_iter = (sizeof(T) == 4 && !plain) ? BPDN_FORM_MFMA : BPDN_FORM_PLAIN;
#endif
        for (T **p : {&x, &y, &u}) *p = dev_alloc<T>(count(), true);
        tk = dev_alloc<T>(tk_count(), true);
        const size_t ldp = (size_t)pl.NB * kRpcaBlk;
        part_g = dev_alloc<double>((size_t)pl.nsplit * ldp * ldp, false);
        g = dev_alloc<double>((size_t)pl.n * pl.n, true);
        part = dev_alloc<double>((size_t)kRpcaSums * pl.nb_iter, false);
        part_s = dev_alloc<double>(1024, false);
        sync();
    }

    void plan(int64_t out[10]) override {
        out[0] = kRpcaKS;
        out[1] = pl.slab;
        out[2] = pl.nsplit;
        out[3] = pl.NB;
        out[4] = pl.KB;
        out[5] = pl.nb_iter;
        out[6] = form_gram;
        out[7] = form_iter;
        out[8] = (int64_t)rpca_gram_lds_bytes();
        out[9] = (int64_t)rpca_iter_lds_bytes<T>(pl);
    }

    void set_signal(const void *S, bool on_device) override {
        SA_REQUIRE(S != nullptr, "rpca: null source");
        if (on_device) {
            sync();      // (no launch of this handle still reads the array in use)
            s = (const T *)S;
        } else {
            if (!s_own) s_own = dev_alloc<T>(count(), false);
            SA_HIP(hipMemcpyAsync(s_own, S, sizeof(T) * count(), hipMemcpyHostToDevice, st));
            sync();      // (the source may be pageable host memory)
            s = s_own;
        }
        const int nb = launch_rpca_sumsq<T>(st, s, (int64_t)count(), part_s);
        const int slots[1] = {SPORCO_AMD_OUT_C2};
        const double ones[1] = {1};
        launch_finalize(st, part_s, nb, 1, 1, slots, ones, false, out_dev);
        sync();
    }

    T *buf(int var) {
        switch (var) {
        case SPORCO_AMD_RPCA_X: return x;
        case SPORCO_AMD_RPCA_Y: return y;
        case SPORCO_AMD_RPCA_U: return u;
        default: throw Error(SPORCO_AMD_EINVAL, "rpca: unknown array id");
        }
    }
    void *var_ptr(int var) override { return buf(var); }
    void upload(int var, const void *src) override {
        SA_REQUIRE(src != nullptr, "rpca: null source");
        SA_HIP(hipMemcpyAsync(buf(var), src, sizeof(T) * count(), hipMemcpyHostToDevice, st));
        sync();
    }
    void download(int var, void *dst) override {
        SA_REQUIRE(dst != nullptr, "rpca: null destination");
        SA_HIP(hipMemcpyAsync(dst, buf(var), sizeof(T) * count(), hipMemcpyDeviceToHost, st));
        sync();
    }
    void gram(int mode, double u_scale, double *G_host) override {
        SA_REQUIRE(s != nullptr, "rpca: S is set first");
        SA_REQUIRE(G_host != nullptr, "rpca: null destination");
        RpcaGramArgs<T> a;
        a.s = s;
        a.y = y;
        a.u = u;
        a.u_scale = (T)u_scale;
        a.mode = mode;
        a.form = form_gram;
        a.part = part_g;
        a.g = g;
        a.p = pl;
        {
            ProfScope ps(prof, PS_RPCA_GRAM);
            launch_rpca_gram<T>(st, a);
        }
        {
            ProfScope ps(prof, PS_RPCA_GRAM_REDUCE);
            launch_rpca_gram_reduce<T>(st, a);
        }
        SA_HIP(hipMemcpyAsync(G_host, g, sizeof(double) * (size_t)pl.n * pl.n, hipMemcpyDeviceToHost, st));
        sync();
    }

    void set_t(const double *T_host) {
        SA_REQUIRE(T_host != nullptr, "rpca: null T");
        stage.assign(tk_count(), T(0));
        for (int k = 0; k < pl.n; ++k)
            for (int i = 0; i < pl.n; ++i) stage[(size_t)k * pl.n16 + i] = (T)T_host[(size_t)k * pl.n + i];
        SA_HIP(hipMemcpyAsync(tk, stage.data(), sizeof(T) * tk_count(), hipMemcpyHostToDevice, st));
        sync();      // (stage is reused)
    }

    void iter(const sporco_amd_rpca_params &p, const double *T_host, double *out_host) override {
        SA_REQUIRE(s != nullptr, "rpca: S is set before the first iteration");
        SA_REQUIRE(p.rho > 0.0 && p.lmbda >= 0.0, "rho must be positive, lambda not negative");
        set_t(T_host);
        RpcaIterArgs<T> a;
        a.s = s;
        a.x = x;
        a.y = y;
        a.u = u;
        a.tk = tk;
        a.rlx = (T)p.rlx;
        a.thr = (T)p.lmbda / (T)p.rho;      // (in the working precision, as rpca.py:185-186 has it)
        a.u_scale = (T)p.u_scale;
        a.form = form_iter;
        a.partials = part;
        a.p = pl;
        {
            ProfScope ps(prof, PS_RPCA_ITER);
            launch_rpca_iter<T>(st, a);
        }
        // (rpca_sums order)
        const int slots[7] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2,
                              SPORCO_AMD_OUT_U2, SPORCO_AMD_OUT_L1, SPORCO_AMD_OUT_L21};
        const double ones[7] = {1, 1, 1, 1, 1, 1, 1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize(st, part, pl.nb_iter, kRpcaSums, 7, slots, ones, false, out_dev);
        }
        read_out(out_host);
    }

    void apply(const double *T_host) override {
        SA_REQUIRE(s != nullptr, "rpca: S is set first");
        set_t(T_host);
        RpcaIterArgs<T> a;
        a.s = s;
        a.x = x;
        a.tk = tk;
        a.apply = 1;
        a.form = form_iter;
        a.p = pl;
        {
            ProfScope ps(prof, PS_RPCA_ITER);
            launch_rpca_iter<T>(st, a);
        }
        sync();
    }
};

RpcaBase *make_rpca(int dtype, int R, int C, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new Rpca<float>(R, C, device, stream);
    if (dtype == SPORCO_AMD_F64) return new Rpca<double>(R, C, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
