// api_cmod.inc -- the handle of CnstrMOD (sporco/admm/cmod.py:21-342); kernels: csc_cmod.h.  It is included by
// csc_api.hip at namespace scope and keeps its stream, sums and buffers through SideBase (csc_impl.h).  Z is (M, K), S (N, K), row-major as NumPy has them: either the
// handle's own copy of a host array or a device pointer read in place.  X, Y, U, S Z^T and the right-hand side are
// (N, M) to the host; the handle keeps them k-major and zero padded, [M4][N16], as bpdn_product reads a left
// operand.  The solve matrix Q = (Z Z^T + rho I)^-1 comes from the host in the handle's precision.
template <typename T> struct Cmod : CmodBase {
    const int N, M;
    const int64_t K;
    const CmodPlan pl;
    int form;                       // BPDN_FORM_MFMA: float32 on the device unless SPORCO_AMD_CMOD_PLAIN is set
    int KB, nb_dfid, nb_iter;
    T *s_own = nullptr, *z_own = nullptr;
    const T *s = nullptr, *z = nullptr;
    T *part_g = nullptr, *sztk = nullptr, *bk = nullptr, *xk = nullptr, *yk = nullptr, *uk = nullptr, *q = nullptr;
    double *g = nullptr, *sztd = nullptr, *part = nullptr, *part_d = nullptr;
    bool have_q = false;
    std::vector<T> stage;

    size_t kmaj() const { return (size_t)pl.M4 * pl.N16; }

    Cmod(int N_, int M_, int64_t K_, int dev, void *stream)
        : CmodBase(dev, stream), N(N_), M(M_), K(K_), pl(cmod_plan(N_, M_, K_)) {
#ifdef SPORCO_AMD_HOSTSIM
        form = BPDN_FORM_PLAIN;
#else
        form = (sizeof(T) == 4 && !Switches::set("SPORCO_AMD_CMOD_PLAIN")) ? BPDN_FORM_MFMA : BPDN_FORM_PLAIN;
#endif
        KB = bpdn_kb<T>(M, N);
        nb_dfid = bpdn_blocks(K, KB);
        nb_iter = pl.M16 / 16;
        for (T **p : {&sztk, &bk, &xk, &yk, &uk}) *p = dev_alloc<T>(kmaj(), true);
        q = dev_alloc<T>((size_t)M * M, false);
        part_g = dev_alloc<T>((size_t)pl.nsplit * pl.RB * kCmodBlk * pl.CB * kCmodBlk, false);
        g = dev_alloc<double>((size_t)M * M, true);
        sztd = dev_alloc<double>((size_t)N * M, true);
        part = dev_alloc<double>((size_t)kCmodSums * nb_iter, false);
        part_d = dev_alloc<double>(nb_dfid, false);
        sync();
    }

    void plan(int64_t out[8]) override {
        out[0] = kCmodKS;
        out[1] = pl.slab;
        out[2] = pl.nsplit;
        out[3] = pl.RB;
        out[4] = pl.CB;
        out[5] = form;
        out[6] = (int64_t)cmod_gram_lds_bytes<T>();
        out[7] = (int64_t)cmod_iter_lds_bytes<T>(N, M);
    }

    // a host (rows, K) array into the handle's own buffer, or a device pointer taken as it is
    void take(const void *src, bool on_device, int rows, T **own, const T **use) {
        SA_REQUIRE(src != nullptr, "cmod: null source");
        if (on_device) {
            sync();      // (no launch of this handle still reads the array in use)
            *use = (const T *)src;
            return;
        }
        if (!*own) *own = dev_alloc<T>((size_t)rows * K, false);
        SA_HIP(hipMemcpyAsync(*own, src, sizeof(T) * (size_t)rows * K, hipMemcpyHostToDevice, st));
        sync();      // (the source may be pageable host memory)
        *use = *own;
    }
    void set_signal(const void *S, bool on_device) override { take(S, on_device, N, &s_own, &s); }
    void set_coef(const void *Z, bool on_device) override {
        SA_REQUIRE(s != nullptr, "cmod: S is set before the coefficients");
        take(Z, on_device, M, &z_own, &z);
        CmodGramArgs<T> a;
        a.z = z;
        a.s = s;
        a.part = part_g;
        a.g = g;
        a.sztd = sztd;
        a.sztk = sztk;
        a.M = M;
        a.N = N;
        a.K = K;
        a.form = form;
        a.p = pl;
        {
            ProfScope ps(prof, PS_CMOD_GRAM);
            launch_cmod_gram<T>(st, a);
        }
        {
            ProfScope ps(prof, PS_CMOD_GRAM_REDUCE);
            launch_cmod_gram_reduce<T>(st, a);
        }
        sync();
    }
    void set_solve(const void *Q) override {
        SA_REQUIRE(Q != nullptr, "cmod: null solve matrix");
        SA_HIP(hipMemcpyAsync(q, Q, sizeof(T) * (size_t)M * M, hipMemcpyHostToDevice, st));
        sync();
        have_q = true;
    }

    virtual T *kbuf(int var) {
        switch (var) {
        case SPORCO_AMD_CMOD_X: return xk;
        case SPORCO_AMD_CMOD_Y: return yk;
        case SPORCO_AMD_CMOD_U: return uk;
        case SPORCO_AMD_CMOD_SZT: return sztk;
        default: throw Error(SPORCO_AMD_EINVAL, "cmod: unknown array id");
        }
    }
    void upload(int var, const void *src) override {
        SA_REQUIRE(src != nullptr, "cmod: null source");
        if (var == SPORCO_AMD_CMOD_G || var == SPORCO_AMD_CMOD_SZTD) {
            const bool isg = var == SPORCO_AMD_CMOD_G;
            SA_HIP(hipMemcpyAsync(isg ? g : sztd, src, sizeof(double) * (size_t)(isg ? M : N) * M, hipMemcpyHostToDevice, st));
            sync();
            return;
        }
        T *dst = kbuf(var);
        const T *h = (const T *)src;
        stage.assign(kmaj(), T(0));
        for (int n = 0; n < N; ++n)
            for (int m = 0; m < M; ++m) stage[(size_t)m * pl.N16 + n] = h[(size_t)n * M + m];
        SA_HIP(hipMemcpyAsync(dst, stage.data(), sizeof(T) * kmaj(), hipMemcpyHostToDevice, st));
        sync();      // (stage is reused)
    }
    void download(int var, void *dst) override {
        SA_REQUIRE(dst != nullptr, "cmod: null destination");
        if (var == SPORCO_AMD_CMOD_G || var == SPORCO_AMD_CMOD_SZTD) {
            const bool isg = var == SPORCO_AMD_CMOD_G;
            SA_HIP(hipMemcpyAsync(dst, isg ? g : sztd, sizeof(double) * (size_t)(isg ? M : N) * M, hipMemcpyDeviceToHost, st));
            sync();
            return;
        }
        const T *src = kbuf(var);
        stage.resize(kmaj());
        SA_HIP(hipMemcpyAsync(stage.data(), src, sizeof(T) * kmaj(), hipMemcpyDeviceToHost, st));
        sync();
        T *h = (T *)dst;
        for (int n = 0; n < N; ++n)
            for (int m = 0; m < M; ++m) h[(size_t)n * M + m] = stage[(size_t)m * pl.N16 + n];
    }
    void launch_dfid(const T *fk) {
        CmodDfidArgs<T> d;
        d.fk = fk;
        d.z = z;
        d.s = s;
        d.M = M;
        d.N = N;
        d.K = K;
        d.KB = KB;
        d.form = form;
        d.partials = part_d;
        ProfScope ps(prof, PS_CMOD_DFID);
        launch_cmod_dfid<T>(st, d);
    }

    void iter(const sporco_amd_cmod_params &p, double *out_host) override {
        SA_REQUIRE(s && z && have_q, "cmod: S, the coefficients and the solve matrix are set before the first iteration");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        CmodArgs<T> a;
        a.q = q;
        a.sztk = sztk;
        a.bk = bk;
        a.xk = xk;
        a.yk = yk;
        a.uk = uk;
        a.rho = (T)p.rho;
        a.rlx = (T)p.rlx;
        a.u_scale = (T)p.u_scale;
        a.zero_mean = p.zero_mean;
        a.geval_y = p.geval_y;
        a.form = form;
        a.M = M;
        a.N = N;
        a.partials = part;
        {
            ProfScope ps(prof, PS_CMOD_RHS);
            launch_cmod_rhs<T>(st, a);
        }
        {
            ProfScope ps(prof, PS_CMOD_ITER);
            launch_cmod_iter<T>(st, a);
        }
        if (p.want_dfid) launch_dfid(p.feval_x ? xk : yk);
        // (cmod_sums order; OUT_AX2 = || X ||^2: the residuals are those of ADMMEqual, on the unrelaxed X)
        const int slots[6] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2,
                              SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_U2, SPORCO_AMD_OUT_CNSTR};
        const int slots_d[1] = {SPORCO_AMD_OUT_DFID};
        const double ones[6] = {1, 1, 1, 1, 1, 1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize2(st, part, nb_iter, kCmodSums, 6, slots, ones, part_d, nb_dfid, 1, p.want_dfid ? 1 : 0, slots_d,
                             ones, out_dev);
        }
        read_out(out_host);
    }

    void dfid(int var, double *out_host) override {
        SA_REQUIRE(s && z, "cmod: S and the coefficients are set first");
        SA_REQUIRE(var == SPORCO_AMD_CMOD_X || var == SPORCO_AMD_CMOD_Y, "cmod: DFid is taken at X or Y");
        launch_dfid(kbuf(var));
        const int slots_d[1] = {SPORCO_AMD_OUT_DFID};
        const double ones[1] = {1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize(st, part_d, nb_dfid, 1, 1, slots_d, ones, false, out_dev);
        }
        read_out(out_host);
    }
};

CmodBase *make_cmod(int dtype, int N, int M, int64_t K, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new Cmod<float>(N, M, K, device, stream);
    if (dtype == SPORCO_AMD_F64) return new Cmod<double>(N, M, K, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
