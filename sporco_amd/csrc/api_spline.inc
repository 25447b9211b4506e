// api_spline.inc -- the handle of SplineL1 (sporco/admm/spline.py:24-291); kernels: csc_spline.h, transforms:
// rfft2 / irfft2 of fft.h on the generic chain.  Like api_tvdc.inc it is included by csc_api.hip at namespace
// scope, below template Csc<T>, and keeps its stream, sums, plans and buffers through SideBase.  S, Y, U and the weight are (H, W, P) arrays in their natural order; XV, RY, RU are
// the same size in the DCT's permuted order (csc_spline.h); the work spectrum is (H, Wf, P).
template <typename T> struct Spl : SplBase {
    const int H, W, Wf;
    const int64_t P;
    int64_t E;                      // H W P
    T *s = nullptr, *x = nullptr, *xv = nullptr, *y = nullptr, *u = nullptr, *ry = nullptr, *ru = nullptr, *wdf = nullptr;
    SplTab<T> *th = nullptr, *tw = nullptr;
    cx<T> *wf = nullptr;
    bool have_wdf = false, have_s = false;
    int sblocks = 1, yblocks = 1, solve_vals = 0;
    double *part_y = nullptr, *part_s = nullptr;

    Spl(int H_, int W_, int64_t P_, int dev, void *stream) : SplBase(dev, stream), H(H_), W(W_), Wf(W_ / 2 + 1), P(P_) {
        E = (int64_t)H * W * P;
        planH.init(H);
        planW.init(W);
        // (the refusal of a line that does not fit a workgroup's LDS comes here, not at the first iteration)
        fft_require_line_fits<T>(planW);
        fft_require_line_fits<T>(planH);
        for (T **p : {&s, &x, &xv, &y, &u, &ry, &ru}) *p = dev_alloc<T>(E, true);
        wf = dev_alloc<cx<T>>((size_t)H * Wf * P, true);
        th = dev_alloc<SplTab<T>>(H, false);
        tw = dev_alloc<SplTab<T>>(W, false);
        launch_spl_tables<T>(st, H, W, th, tw);
        sblocks = spl_solve_blocks(solve_args(T(1)));
        yblocks = kSplMaxBlocks;      // (spl_ystep and, when S is set, spl_sumsq leave their partials here)
        part_y = dev_alloc<double>(kSplYstepSums * yblocks, false);
        part_s = dev_alloc<double>(kSplSolveSums * sblocks, false);
        sync();
    }

    void plan(int64_t out[4]) override {
        // planes per access of the kernels (2: 16 bytes of spectrum, 8 of image in float32), row pairs of
        // spl_solve, its workgroups and those of spl_ystep
        out[0] = (sizeof(T) == 4 && P % 2 == 0) ? 2 : 1;
        out[1] = H / 2 + 1;
        out[2] = sblocks;
        out[3] = spl_ystep_blocks<T>(H, W, P);
    }

    SplSolveArgs<T> solve_args(T lr) {
        SplSolveArgs<T> a;
        a.wf = wf;
        a.th = th;
        a.tw = tw;
        a.H = H;
        a.W = W;
        a.Wf = Wf;
        a.P = P;
        a.lr = lr;
        a.partials = part_s;
        return a;
    }

    T *var_buf(int var) {
        switch (var) {
        case SPORCO_AMD_SPL_S: return s;
        case SPORCO_AMD_SPL_Y: return y;
        case SPORCO_AMD_SPL_U: return u;
        case SPORCO_AMD_SPL_WDF: return wdf;
        default: throw Error(SPORCO_AMD_EINVAL, "spline: unknown array id");
        }
    }
    void upload(int var, const void *src, bool on_device) override {
        SA_REQUIRE(var != SPORCO_AMD_SPL_X, "spline: X is the result of the x step, it is not set");
        if (var == SPORCO_AMD_SPL_WDF) {
            have_wdf = src != nullptr;
            if (!have_wdf) return;
            if (!wdf) wdf = dev_alloc<T>(E, false);
        }
        SA_REQUIRE(src != nullptr, "spline: null source");
        SA_HIP(hipMemcpyAsync(var_buf(var), src, sizeof(T) * E, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                              st));
        if (var == SPORCO_AMD_SPL_S) {
            // || c ||^2 = || S ||^2 of the primal normaliser is constant: formed here, on the device, into a
            // slot of out_dev that no later finalize writes, so every read of the sums carries it
            const int nb = launch_spl_sumsq<T>(st, s, E, part_y);
            const int slot = SPORCO_AMD_OUT_C2;
            const double one = 1.0;
            launch_finalize(st, part_y, nb, 1, 1, &slot, &one, false, out_dev);
            have_s = true;
        }
        // the permuted arrays of the next right-hand side
        if (var == SPORCO_AMD_SPL_S || var == SPORCO_AMD_SPL_Y) launch_spl_permute<T>(st, y, s, ry, H, W, P, false);
        if (var == SPORCO_AMD_SPL_U) launch_spl_permute<T>(st, u, nullptr, ru, H, W, P, false);
        sync();      // (the source may be pageable host memory, or a device array the caller frees next)
    }
    void download(int var, void *dst, bool on_device) override {
        SA_REQUIRE(dst != nullptr, "spline: null destination");
        const T *src;
        if (var == SPORCO_AMD_SPL_X) {
            launch_spl_permute<T>(st, xv, nullptr, x, H, W, P, true);
            src = x;
        } else {
            src = var_buf(var);
            SA_REQUIRE(src != nullptr, "spline: the weight is a scalar");
        }
        SA_HIP(hipMemcpyAsync(dst, src, sizeof(T) * E, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        sync();
    }
    // the x step: X = idct(Gamma dct(Y + S - u_scale U)), left in the permuted order of the transform
    void xstep(const sporco_amd_spl_params &p) override {
        SA_REQUIRE(have_s, "spline: S is set before the first x step");
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        {
            ProfScope ps(prof, PS_SPL_RFFT2);
            rfft2<T>(st, planW, planH, ry, ru, (T)p.u_scale, wf, H, W, P);
        }
        SplSolveArgs<T> a = solve_args((T)((T)p.lmbda / (T)p.rho));
        a.want_reg = p.want_stats ? 1 : 0;
        a.want_lsc = p.lin_solve_check ? 1 : 0;
        solve_vals = a.want_lsc ? 4 : (a.want_reg ? 1 : 0);
        {
            ProfScope ps(prof, PS_SPL_SOLVE);
            launch_spl_solve<T>(st, a);
        }
        {
            ProfScope ps(prof, PS_SPL_IRFFT2);
            irfft2<T>(st, planW, planH, wf, wf, xv, H, W, P);
        }
    }
    // relax + y step + u step and the permuted arrays of the next right-hand side in one launch, the sums of
    // both steps in one reduction, one host read
    void ystep(const sporco_amd_spl_params &p, double *out_host) override {
        SA_REQUIRE(p.rho > 0.0, "rho must be positive");
        SplArgs<T> a;
        a.s = s;
        a.xv = xv;
        a.y = y;
        a.u = u;
        a.ry = ry;
        a.ru = ru;
        a.wdf = have_wdf ? wdf : nullptr;
        a.wdf_s = (T)p.wdf;
        a.rho = (T)p.rho;
        a.rlx = (T)p.rlx;
        a.u_scale = (T)p.u_scale;
        a.geval_y = p.geval_y;
        a.H = H;
        a.W = W;
        a.P = P;
        a.partials = part_y;
        int nb;
        {
            ProfScope ps(prof, PS_SPL_YSTEP);
            nb = launch_spl_ystep<T>(st, a);
        }
        // (OUT_RGR = sum (alpha Xhat)^2, twice Reg; OUT_S2 = || Y - Yprev ||^2, rho applied by the host)
        const int slots_y[6] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2,
                                SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_U2, SPORCO_AMD_OUT_DFID};
        const int slots_s[4] = {SPORCO_AMD_OUT_RGR, SPORCO_AMD_OUT_XRRS_D2, SPORCO_AMD_OUT_XRRS_AX2,
                                SPORCO_AMD_OUT_XRRS_B2};
        const double ones[6] = {1, 1, 1, 1, 1, 1};
        {
            ProfScope ps(prof, PS_FINALIZE);
            launch_finalize2(st, part_y, nb, kSplYstepSums, 6, slots_y, ones, part_s, sblocks, kSplSolveSums, solve_vals,
                             slots_s, ones, out_dev);
        }
        solve_vals = 0;
        read_out(out_host);
    }
};

SplBase *make_spl(int dtype, int H, int W, int64_t P, int device, void *stream) {
    if (dtype == SPORCO_AMD_F32) return new Spl<float>(H, W, P, device, stream);
    if (dtype == SPORCO_AMD_F64) return new Spl<double>(H, W, P, device, stream);
    throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}

// The stateless DCT-II / inverse DCT-II over axes (0, 1) of an (H, W, P) array, host or device pointers.
// Stateless means just that: every call allocates its two work arrays, the work spectrum and the tables, builds
// the two transform plans, works on the null stream of the current device and synchronises the device before it
// returns -- the cost of a handle creation per call, as the other stateless primitives of csc_prims.hip pay it.
// Code that transforms the same shape repeatedly keeps a handle (Spl above keeps plans, tables and buffers);
// a cached context per (dtype, H, W) for this entry point is the natural follow-up.
template <typename T> void spl_dct(int H, int W, int64_t P, const void *in, void *out, bool inverse, bool on_device) {
    const int64_t E = (int64_t)H * W * P, F = (int64_t)H * (W / 2 + 1) * P;
    struct Bufs {
        T *a = nullptr, *b = nullptr;
        cx<T> *wf = nullptr;
        SplTab<T> *th = nullptr, *tw = nullptr;
        FftPlan pw, ph;
        ~Bufs() {
            (void)hipDeviceSynchronize();
            for (void *p : {(void *)a, (void *)b, (void *)wf, (void *)th, (void *)tw})
                if (p) (void)hipFree(p);
            pw.destroy();
            ph.destroy();
        }
    } m;
    m.ph.init(H);
    m.pw.init(W);
    fft_require_line_fits<T>(m.pw);
    fft_require_line_fits<T>(m.ph);
    SA_HIP(hipMalloc((void **)&m.a, sizeof(T) * E));
    SA_HIP(hipMalloc((void **)&m.b, sizeof(T) * E));
    SA_HIP(hipMalloc((void **)&m.wf, sizeof(cx<T>) * F));
    SA_HIP(hipMalloc((void **)&m.th, sizeof(SplTab<T>) * H));
    SA_HIP(hipMalloc((void **)&m.tw, sizeof(SplTab<T>) * W));
    launch_spl_tables<T>(nullptr, H, W, m.th, m.tw);
    const T *src = (const T *)in;
    if (!on_device) {
        SA_HIP(hipMemcpy(m.a, in, sizeof(T) * E, hipMemcpyHostToDevice));
        src = m.a;
    }
    T *dst = on_device ? (T *)out : m.a;
    SplSolveArgs<T> a;
    a.wf = m.wf;
    a.th = m.th;
    a.tw = m.tw;
    a.H = H;
    a.W = W;
    a.Wf = W / 2 + 1;
    a.P = P;
    if (!inverse) {
        launch_spl_permute<T>(nullptr, src, nullptr, m.b, H, W, P, false);
        rfft2<T>(nullptr, m.pw, m.ph, m.b, nullptr, T(0), m.wf, H, W, P);
        a.xr = dst;
        launch_dct_post<T>(nullptr, a);
    } else {
        a.xr = const_cast<T *>(src);
        launch_dct_pre<T>(nullptr, a);
        irfft2<T>(nullptr, m.pw, m.ph, m.wf, m.wf, m.b, H, W, P);
        launch_spl_permute<T>(nullptr, m.b, nullptr, dst, H, W, P, true);
    }
    SA_HIP(hipDeviceSynchronize());
    if (!on_device) SA_HIP(hipMemcpy(out, m.a, sizeof(T) * E, hipMemcpyDeviceToHost));
}

void spl_dct_dispatch(int dtype, int H, int W, int64_t P, const void *in, void *out, bool inverse, bool on_device) {
    if (dtype == SPORCO_AMD_F32) spl_dct<float>(H, W, P, in, out, inverse, on_device);
    else if (dtype == SPORCO_AMD_F64) spl_dct<double>(H, W, P, in, out, inverse, on_device);
    else throw Error(SPORCO_AMD_EINVAL, "dtype must be SPORCO_AMD_F32 or SPORCO_AMD_F64");
}
