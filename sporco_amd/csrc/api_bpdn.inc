// api_bpdn.inc -- the handle of BPDN / BPDNJoint / ElasticNet / BPDNProjL1 (sporco/admm/bpdn.py:24-914); kernels: csc_bpdn.h.
// It is included by csc_api.hip at namespace scope; the stream, the sums, the profiler and the ownership of every
// buffer are SideBase's (csc_impl.h).  S is (N, K); X, Y, U, D^T S, the weight,
// Z and the saved right-hand side are (M, K), all row-major as NumPy has them.  The dictionary and the solve
// matrix P = (D^T D + c I)^-1 come from the host in the handle's precision; the handle keeps them k-major and zero
// padded, as bpdn_product reads them.
template <typename T> struct Bpdn : BpdnBase {
    const int N, M, KB;
    const int64_t K;
    int form;                       // BPDN_FORM_MFMA: float32 on the device unless SPORCO_AMD_BPDN_PLAIN is set
    int M4, N4, M16, N16, nb;
    T *s = nullptr, *dts = nullptr, *x = nullptr, *y = nullptr, *u = nullptr, *z = nullptr, *bsave = nullptr, *wl1 = nullptr;
    T *pk = nullptr, *dk = nullptr, *dtk = nullptr, *rowf = nullptr;
    bool have_wl1 = false, have_s = false, have_d = false, have_p = false;
    double *part = nullptr, *part_lsc = nullptr, *rowp = nullptr, *rowpx = nullptr;
    std::vector<T> stage;

    Bpdn(int N_, int M_, int64_t K_, int dev, void *stream)
        : BpdnBase(dev, stream), N(N_), M(M_), KB(bpdn_kb<T>(M_, N_)), K(K_) {
#ifdef SPORCO_AMD_HOSTSIM
        form = BPDN_FORM_PLAIN;
#else
        form = (sizeof(T) == 4 && !Switches::set("SPORCO_AMD_BPDN_PLAIN")) ? BPDN_FORM_MFMA : BPDN_FORM_PLAIN;
#endif
        M4 = bpdn_up(M, 4);
        N4 = bpdn_up(N, 4);
        M16 = bpdn_up(M, 16);
        N16 = bpdn_up(N, 16);
        nb = bpdn_blocks(K, KB);
        s = dev_alloc<T>((size_t)N * K, true);
        for (T **p : {&dts, &x, &y, &u}) need(p);
        pk = dev_alloc<T>((size_t)M4 * M16, false);
        dk = dev_alloc<T>((size_t)N4 * M16, false);
        dtk = dev_alloc<T>((size_t)M4 * N16, false);
        part = dev_alloc<double>((size_t)kBpdnSums * nb, false);
        sync();
    }

    void plan(int64_t out[4]) override {
        out[0] = KB;
        out[1] = nb;
        out[2] = form;
        out[3] = (int64_t)bpdn_lds_bytes<T>(M, N);
    }

    // an (M, K) array made on first use, zeroed
    void need(T **p) {
        if (!*p) *p = dev_alloc<T>((size_t)M * K, true);
    }

    BpdnArgs<T> args() {
        BpdnArgs<T> a;
        a.pk = pk;
        a.dk = dk;
        a.dtk = dtk;
        a.s = s;
        a.dts = dts;
        a.x = x;
        a.y = y;
        a.u = u;
        a.M = M;
        a.N = N;
        a.K = K;
        a.KB = KB;
        a.form = form;
        a.partials = part;
        return a;
    }

    // dst [rows4][cols16] <- src (rows, cols) row-major (transpose: src is (cols, rows)), zero padded
    void upload_padded(T *dst, const T *src, int rows, int cols, int rows4, int cols16, bool transpose) {
        stage.assign((size_t)rows4 * cols16, T(0));
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c)
                stage[(size_t)r * cols16 + c] = transpose ? src[(size_t)c * rows + r] : src[(size_t)r * cols + c];
        SA_HIP(hipMemcpyAsync(dst, stage.data(), sizeof(T) * stage.size(), hipMemcpyHostToDevice, st));
        sync();      // (stage is reused)
    }
    void form_dts() {
        if (!(have_s && have_d)) return;
        ProfScope ps(prof, PS_BPDN_DTS);
        launch_bpdn_dts<T>(st, args());
    }
    void set_dict(const void *D) override {
        SA_REQUIRE(D != nullptr, "bpdn: null dictionary");
        const T *d = (const T *)D;
        upload_padded(dk, d, N, M, N4, M16, false);      // k = n, rows of the result = m
        upload_padded(dtk, d, M, N, M4, N16, true);      // k = m, rows of the result = n
        have_d = true;
        form_dts();
        sync();
    }
    void set_solve(const void *P) override {
        SA_REQUIRE(P != nullptr, "bpdn: null solve matrix");
        // (k-major = the transpose; P is symmetric up to the rounding of its inverse, and it is the transpose that
        // bpdn_product multiplies by in row-major terms: out[i] = sum_k P[i][k] b[k])
        upload_padded(pk, (const T *)P, M, M, M4, M16, true);
        have_p = true;
    }

    virtual T *var_buf(int var) {
        switch (var) {
        case SPORCO_AMD_BPDN_S: return s;
        case SPORCO_AMD_BPDN_X: return x;
        case SPORCO_AMD_BPDN_Y: return y;
        case SPORCO_AMD_BPDN_U: return u;
        case SPORCO_AMD_BPDN_WL1: return wl1;
        case SPORCO_AMD_BPDN_DTS: return dts;
        default: throw Error(SPORCO_AMD_EINVAL, "bpdn: unknown array id");
        }
    }
    void *var_ptr(int var) override { return var_buf(var); }
    virtual size_t var_bytes(int var) const { return sizeof(T) * (size_t)(var == SPORCO_AMD_BPDN_S ? N : M) * K; }
    void upload(int var, const void *src) override {
        // (X and D^T S are results: setting them only prefills what the next iteration / set_dict overwrites)
        if (var == SPORCO_AMD_BPDN_WL1) {
            have_wl1 = src != nullptr;
            if (!have_wl1) return;
            need(&wl1);
        }
        SA_REQUIRE(src != nullptr, "bpdn: null source");
        SA_HIP(hipMemcpyAsync(var_buf(var), src, var_bytes(var), hipMemcpyHostToDevice, st));
        if (var == SPORCO_AMD_BPDN_S) {
            have_s = true;
            form_dts();
        }
        sync();      // (the source may be pageable host memory)
    }
    void download(int var, void *dst) override {
        SA_REQUIRE(dst != nullptr, "bpdn: null destination");
        const T *src = var_buf(var);
        SA_REQUIRE(src != nullptr, "bpdn: the weight is a scalar");
        SA_HIP(hipMemcpyAsync(dst, src, var_bytes(var), hipMemcpyDeviceToHost, st));
        sync();
    }
    void iter(const sporco_amd_bpdn_params &p, double *out_host) override {
        SA_REQUIRE(have_s && have_d && have_p, "bpdn: S, the dictionary and the solve matrix are set before the first iteration");
        SA_REQUIRE(p.rho > 0.0 && p.c > 0.0, "rho must be positive");
        BpdnArgs<T> a = args();
        a.wl1 = have_wl1 ? wl1 : nullptr;
        a.wl1_s = (T)p.wl1;
        a.rho = (T)p.rho;
        a.lr = (T)p.lmbda / (T)p.rho;
        a.rlx = (T)p.rlx;
        a.u_scale = (T)p.u_scale;
        a.c = (T)p.c;
        a.nonneg = p.nonneg;
        a.feval_x = p.feval_x;
        a.geval_y = p.geval_y;
        a.joint = p.joint;
        a.proj_l1 = p.proj_l1;
        if (p.proj_l1) {
            SA_REQUIRE(!p.joint && p.lmbda >= 0.0, "bpdn: proj_l1 takes gamma >= 0 in lmbda and no joint term");
            a.gamma = p.lmbda;
            a.lr = T(0);
        }
        a.want_x = (p.want_x || p.lin_solve_check || p.joint) ? 1 : 0;
        if (p.lin_solve_check) {
            need(&bsave);
            if (!part_lsc) part_lsc = dev_alloc<double>((size_t)kBpdnLscSums * nb, false);
            a.bsave = bsave;
        }
        if (p.joint) {
            need(&z);
            if (!rowp) rowp = dev_alloc<double>((size_t)M * nb, false);
            if (!rowf) rowf = dev_alloc<T>(M, false);
            if (!p.geval_y && !rowpx) rowpx = dev_alloc<double>((size_t)M * nb, false);
            a.z = z;
            a.rowp = rowp;
            a.rowf = rowf;
            a.rowpx = p.geval_y ? nullptr : rowpx;
        }
        {
            ProfScope ps(prof, PS_BPDN_ITER);
            launch_bpdn_iter<T>(st, a);
        }
        if (p.joint) {
            {
                ProfScope ps(prof, PS_BPDN_JOINT_ROWS);
                launch_bpdn_joint_rows<T>(st, rowp, nb, M, 0, (T)p.mu / (T)p.rho, rowf, nullptr, 0);
                // RegL21 at X (gEvalY off): the row norms of X
                if (!p.geval_y) launch_bpdn_joint_rows<T>(st, rowpx, nb, M, 1, T(0), nullptr, out_dev, SPORCO_AMD_OUT_L21);
            }
            {
                ProfScope ps(prof, PS_BPDN_JOINT_APPLY);
                launch_bpdn_joint_apply<T>(st, a);
            }
            if (p.geval_y) {
                ProfScope ps(prof, PS_BPDN_JOINT_ROWS);
                launch_bpdn_joint_rows<T>(st, rowp, nb, M, 1, T(0), nullptr, out_dev, SPORCO_AMD_OUT_L21);
            }
        }
        int lsc_vals = 0;
        if (p.lin_solve_check) {
            BpdnArgs<T> l = a;
            l.partials = part_lsc;
            ProfScope ps(prof, PS_BPDN_LSC);
            launch_bpdn_lsc<T>(st, l);
            lsc_vals = kBpdnLscSums;
        }
        // (bpdn_sums order; OUT_AX2 = || X ||^2: the residuals are those of ADMMEqual, on the unrelaxed X)
        // projection mode: the eighth sum, BPDN_CNSTR
        const int slots[8] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2, SPORCO_AMD_OUT_S2,
                              SPORCO_AMD_OUT_U2, SPORCO_AMD_OUT_DFID, SPORCO_AMD_OUT_L1, SPORCO_AMD_OUT_BPDN_CNSTR};
        const int slots_l[3] = {SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2, SPORCO_AMD_OUT_XRRS_B2};
        const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize2(st, part, nb, kBpdnSums, p.proj_l1 ? 8 : 7, slots, ones, part_lsc ? part_lsc : part, nb,
                             kBpdnLscSums, lsc_vals, slots_l, ones, out_dev);
        }
        read_out(out_host);
    }
};

BpdnBase *make_bpdn(int dtype, int N, int M, int64_t K, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new Bpdn<float>(N, M, K, device, stream);
    if (dtype == SPORCO_AMD_F64) return new Bpdn<double>(N, M, K, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
