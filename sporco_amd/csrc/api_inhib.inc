// api_inhib.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvBPDNInhib (sporco/admm/cbpdnin.py): the inhibition state of a handle and its
// per-iteration update (csc_inhib.h).
    // While inh_active, the handle's L1-weight array (wl1 / wl1_buf) holds the thresholds
    // T = lmbda w0 + mu wml + gamma wms, E elements; w0 is the caller's L1Weight, moved aside.
    bool inh_active = false, inh_self = false;
    Weight<T> inh_w0;
    T *inh_w0_buf = nullptr;
    T *inh_taps = nullptr;      // taps_h (nth), taps_w (ntw)
    int inh_nth = 1, inh_ntw = 1, inh_ng = 0;
    T inh_h0 = T(0);
    int *inh_idx = nullptr;     // row_ptr (Ng + 1), row_k (nnz), col_ptr (K + 1), col_g (nnz)
    T *inh_val = nullptr;       // row_v (nnz), col_v (nnz), col_sum (K)
    int inh_nnz = 0;
    double *inh_part = nullptr;
    int64_t inh_part_cap = 0;
    InhibPlan inh_plan;

    void inhib_free_tables() {
        for (void *p : {(void *)inh_taps, (void *)inh_idx, (void *)inh_val})
            if (p) (void)hipFree(p);
        inh_taps = nullptr;
        inh_idx = nullptr;
        inh_val = nullptr;
    }
    // the L1-weight array is being replaced (set_weight): the thresholds go with it
    void inhib_drop() {
        if (!inh_active) return;
        sync();
        inh_active = false;
        if (inh_w0_buf) SA_HIP(hipFree(inh_w0_buf));
        inh_w0_buf = nullptr;
        inh_w0 = Weight<T>();
        inhib_free_tables();
    }
    void inhib_release() {
        if (inh_w0_buf) (void)hipFree(inh_w0_buf);
        if (inh_part) (void)hipFree(inh_part);
        inh_w0_buf = nullptr;
        inh_part = nullptr;
        inhib_free_tables();
    }

    void inhib_setup(const double *Wg, int Ng, const double *taps_h, int nth, const double *taps_w, int ntw,
                     bool want_self, double lmbda) override {
        SA_REQUIRE(Cd == 1 && depth == 1 && !cplx, "inhibition: single-channel real dictionary, no volume handle");
        SA_REQUIRE(Ng >= 0 && (Ng == 0 || Wg != nullptr), "inhibition: Ng groups need a grouping matrix");
        const bool lateral = Ng > 0;
        SA_REQUIRE(lateral || want_self, "inhibition: neither a lateral nor a self term");
        before_state_change();
        sync();
        int nnz_plan = 0;
        for (int64_t i = 0; lateral && i < (int64_t)Ng * Ku; ++i) nnz_plan += Wg[i] != 0.0;
        inh_plan = inhib_plan<T>(H, W, CN, K, nth, ntw, Ng, nnz_plan);   // (validates the window lengths)
        if (!inh_active) {
            // the caller's L1Weight moves aside; the handle's array becomes the thresholds
            inh_w0 = wl1;
            inh_w0_buf = wl1_buf;
            wl1_buf = nullptr;
            SA_HIP(hipMalloc((void **)&wl1_buf, sizeof(T) * E));
            wl1 = Weight<T>();
            wl1.ptr = wl1_buf;
            int64_t stride = 1;
            const int64_t shape[5] = {H, W, C, N, K};
            for (int i = 4; i >= 0; --i) {
                wl1.stride[i] = stride;
                stride *= shape[i];
            }
        }
        inhib_free_tables();
        inh_nth = nth;
        inh_ntw = ntw;
        inh_ng = Ng;
        inh_self = want_self;
        inh_h0 = (T)(taps_h[nth / 2] * taps_w[ntw / 2]);
        std::vector<T> taps((size_t)nth + ntw);
        for (int i = 0; i < nth; ++i) taps[i] = (T)taps_h[i];
        for (int i = 0; i < ntw; ++i) taps[nth + i] = (T)taps_w[i];
        SA_HIP(hipMalloc((void **)&inh_taps, sizeof(T) * taps.size()));
        SA_HIP(hipMemcpy(inh_taps, taps.data(), sizeof(T) * taps.size(), hipMemcpyHostToDevice));
        inh_nnz = 0;
        if (lateral) {
            // Wg has Ku columns (the caller's filters); a padding filter belongs to no group
            std::vector<int> row_ptr(Ng + 1, 0), row_k, col_ptr(K + 1, 0), col_g;
            std::vector<T> row_v, col_v, col_sum((size_t)K, T(0));
            for (int g = 0; g < Ng; ++g) {
                for (int k = 0; k < Ku; ++k) {
                    const double v = Wg[(int64_t)g * Ku + k];
                    if (v == 0.0) continue;
                    row_k.push_back(k);
                    row_v.push_back((T)v);
                }
                row_ptr[g + 1] = (int)row_k.size();
            }
            for (int k = 0; k < K; ++k) {
                double cs = 0.0;
                for (int g = 0; g < Ng && k < Ku; ++g) {
                    const double v = Wg[(int64_t)g * Ku + k];
                    cs += v;
                    if (v == 0.0) continue;
                    col_g.push_back(g);
                    col_v.push_back((T)v);
                }
                col_sum[k] = (T)cs;
                col_ptr[k + 1] = (int)col_g.size();
            }
            inh_nnz = (int)row_k.size();
            std::vector<int> idx;
            idx.insert(idx.end(), row_ptr.begin(), row_ptr.end());
            idx.insert(idx.end(), row_k.begin(), row_k.end());
            idx.insert(idx.end(), col_ptr.begin(), col_ptr.end());
            idx.insert(idx.end(), col_g.begin(), col_g.end());
            std::vector<T> val;
            val.insert(val.end(), row_v.begin(), row_v.end());
            val.insert(val.end(), col_v.begin(), col_v.end());
            val.insert(val.end(), col_sum.begin(), col_sum.end());
            SA_HIP(hipMalloc((void **)&inh_idx, sizeof(int) * idx.size()));
            SA_HIP(hipMalloc((void **)&inh_val, sizeof(T) * val.size()));
            SA_HIP(hipMemcpy(inh_idx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice));
            SA_HIP(hipMemcpy(inh_val, val.data(), sizeof(T) * val.size(), hipMemcpyHostToDevice));
        }
        // only the live weight arrays exist; they start at zero (cbpdnin.py:229)
        if (lateral) SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_WML), 0, sizeof(T) * E, st));
        if (want_self) SA_HIP(hipMemsetAsync(rv(SPORCO_AMD_VAR_WMS), 0, sizeof(T) * E, st));
        if (inh_plan.blocks > inh_part_cap) {
            if (inh_part) SA_HIP(hipFree(inh_part));
            inh_part = nullptr;
            SA_HIP(hipMalloc((void **)&inh_part, sizeof(double) * 4 * inh_plan.blocks));
            inh_part_cap = inh_plan.blocks;
        }
        {
            ProfScope ps(prof, PS_OTHER);
            launch_inhib_init<T>(st, wl1_buf, inh_w0, (T)lmbda, d5());
        }
        sync();
        inh_active = true;
    }

    void inhib_update(const sporco_amd_inhib_params &p, double *out_dev) override {
        SA_REQUIRE(inh_active, "inhib_update without inhib_setup");
        const bool lateral = p.mu > 0.0, self = p.gamma > 0.0;
        SA_REQUIRE(!lateral || inh_ng > 0, "inhib_update: mu > 0 needs a grouping matrix (inhib_setup)");
        SA_REQUIRE(!self || inh_self, "inhib_update: gamma > 0 needs the self term (inhib_setup)");
        // X of the iteration in its array, the iterate as (Y, U) -- derived, where it is held as
        // V = AX + U, with the thresholds that produced it, before they are rewritten below
        // (the row spectrum a fused iteration may have emitted for the next one does not depend on
        // the thresholds and stays valid: no before_state_change())
        before_read(SPORCO_AMD_VAR_X);
        ensure_yu();
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        InhibArgs<T> a;
        a.x = rv(SPORCO_AMD_VAR_X);
        a.g = (p.flags & F_GEVAL_Y) ? rv(SPORCO_AMD_VAR_Y) : a.x;
        a.wml = lateral ? rv(SPORCO_AMD_VAR_WML) : nullptr;
        a.wms = self ? rv(SPORCO_AMD_VAR_WMS) : nullptr;
        a.t = wl1_buf;
        a.w0 = inh_w0;
        a.taps_h = inh_taps;
        a.taps_w = inh_taps + inh_nth;
        a.nth = inh_nth;
        a.ntw = inh_ntw;
        if (lateral) {
            a.row_ptr = inh_idx;
            a.row_k = a.row_ptr + inh_ng + 1;
            a.col_ptr = a.row_k + inh_nnz;
            a.col_g = a.col_ptr + K + 1;
            a.row_v = inh_val;
            a.col_v = a.row_v + inh_nnz;
            a.col_sum = a.col_v + inh_nnz;
            a.Ng = inh_ng;
            a.nnz = inh_nnz;
        }
        a.lmbda = (T)p.lmbda;
        a.mu = (T)p.mu;
        a.gamma = (T)p.gamma;
        a.smooth = (T)p.smooth;
        a.h0 = inh_h0;
        a.H = H;
        a.W = W;
        a.C = C;
        a.N = N;
        a.K = K;
        a.partials = inh_part;
        // (without a lateral term the tile needs no group sums: the plan of the set-up still fits)
        int64_t nb;
        {
            ProfScope ps(prof, PS_INHIB);
            nb = launch_inhib_update<T>(st, a, inh_plan);
        }
        const int slots[3] = {SPORCO_AMD_OUT_L1, SPORCO_AMD_OUT_L21, SPORCO_AMD_OUT_RGR};
        const double scales[3] = {1, 1, 1};
        finalize(inh_part, (int)nb, 4, 3, slots, scales, out_dev);
    }
