// api_projl1.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): ConvBPDNProjL1 (sporco/admm/cbpdn.py:1220-1395): the ConvBPDN x step followed by the
// projection of AX + U onto one l1 ball per image (csc_projl1.h).
    // Two searches live on a handle, each with the thresholds of its previous call as the next call's
    // first guess: [0] on v = AX + U (the y step), [1] on the variable the constraint measure is
    // evaluated at (X, or the new Y under AuxVarObj).
    double *pl_ws[2] = {nullptr, nullptr};
    static constexpr int kProjL1FirstPasses = 3, kProjL1MorePasses = 2;

    void projl1_release() {
        for (double *&w : pl_ws) {
            if (w) (void)hipFree(w);
            w = nullptr;
        }
    }

    ProjL1Geom projl1_handle_geom() const { return projl1_geom(sizeof(T), (int64_t)H * W * C, N, K, true); }

    // search [0] (restart, or `more` further passes), the apply pass and its five sums; the count of
    // images still searching and the passes taken go to OUT_CGIT / OUT_CGN
    void projl1_ystep_launches(const sporco_amd_admm_params &p, double gamma, const ProjL1Geom &g, bool restart,
                               double *out_dev) {
        ProjL1Args<T> a;
        a.x = rv(SPORCO_AMD_VAR_X);
        a.y = rv(SPORCO_AMD_VAR_Y);
        a.u = rv(SPORCO_AMD_VAR_U);
        a.gamma = gamma;
        a.rlx = (T)p.rlx;
        a.us = (T)p.u_scale;
        a.flags = p.flags;
        a.d = d5();
        a.dH = p.dH;
        a.dW = p.dW;
        a.ws = pl_ws[0];
        if (restart) {
            // the first pass runs on every image and reads x, u (and y under relaxation) whole: timed on its
            // own (with the three small launches about it: init, decide, count)
            ProfScope ps(prof, PS_PROJL1_PASS0);
            launch_projl1_search<T>(st, a, g, 1, true);
        }
        {
            ProfScope ps(prof, PS_PROJL1_SEARCH);
            launch_projl1_search<T>(st, a, g, restart ? kProjL1FirstPasses - 1 : kProjL1MorePasses, false);
        }
        int nb;
        {
            ProfScope ps(prof, PS_PROJL1_APPLY);
            nb = launch_projl1_apply<T>(st, a, g, part_b);
        }
        finalize_post(part_b, nb, 5, true, out_dev);
        const double *cnt = projl1_counter(pl_ws[0], g);
        SA_HIP(hipMemcpyAsync(out_dev + SPORCO_AMD_OUT_CGIT, cnt, sizeof(double), hipMemcpyDeviceToDevice, st));
        SA_HIP(hipMemcpyAsync(out_dev + SPORCO_AMD_OUT_CGN, cnt + 1, sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    // search [1] on gv and the constraint measure into OUT_L1; its count and passes go to OUT_CNSTR /
    // OUT_RGRX
    void projl1_cnstr_launches(const T *gv, double gamma, const ProjL1Geom &g, bool restart, double *out_dev) {
        ProjL1Args<T> a;
        a.x = gv;
        a.gamma = gamma;
        a.ws = pl_ws[1];
        {
            ProfScope ps(prof, PS_PROJL1_SEARCH);
            launch_projl1_search<T>(st, a, g, restart ? kProjL1FirstPasses : kProjL1MorePasses, restart);
        }
        int nb;
        {
            ProfScope ps(prof, PS_PROJL1_CNSTR);
            nb = launch_projl1_cnstr<T>(st, a, g, part_a);
        }
        const int slots[1] = {SPORCO_AMD_OUT_L1};
        const double scales[1] = {1};
        finalize(part_a, nb, 1, 1, slots, scales, out_dev);
        const double *cnt = projl1_counter(pl_ws[1], g);
        SA_HIP(hipMemcpyAsync(out_dev + SPORCO_AMD_OUT_CNSTR, cnt, sizeof(double), hipMemcpyDeviceToDevice, st));
        SA_HIP(hipMemcpyAsync(out_dev + SPORCO_AMD_OUT_RGRX, cnt + 1, sizeof(double), hipMemcpyDeviceToDevice, st));
    }

    void projl1_iter(const sporco_amd_admm_params &pin, double gamma, double *out_dev, double *out_host) override {
        if (depth > 1 || comm_user || cplx)
            throw Error(SPORCO_AMD_EUNSUPPORTED, "projl1_iter: no volume handle, no communicator, real data");
        SA_REQUIRE(gamma >= 0.0, "gamma must not be negative");
        SA_REQUIRE(pin.rho > 0.0, "rho must be positive");
        const ProjL1Geom g = projl1_handle_geom();
        for (double *&w : pl_ws)
            if (!w) {
                SA_HIP(hipMalloc((void **)&w, sizeof(double) * g.workspace_doubles()));
                projl1_reset(st, w, g);
            }
        sporco_amd_admm_params p = pin;
        p.lmbda = 0.0;          // (no l1 term: the x step is ConvBPDN's)
        p.mu = 0.0;
        p.flags &= ~(uint32_t)(F_JOINT | F_GRADREG | F_AMS);
        before_state_change();
        SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
        xstep_impl(p, out_dev);
        const bool want = p.flags & F_OBJ, at_y = p.flags & F_GEVAL_Y;
        projl1_ystep_launches(p, gamma, g, true, out_dev);
        // (Under AuxVarObj the constraint search reads the new Y.  It is enqueued here without knowing whether
        // the y search has ended; if it has not, the apply pass left Y as it was, this search ran on the old Y
        // -- three passes and a read pass wasted, and its threshold kept as the next first guess -- and the
        // loop below runs it again from the start on the new Y.)
        if (want) projl1_cnstr_launches(at_y ? rv(SPORCO_AMD_VAR_Y) : rv(SPORCO_AMD_VAR_X), gamma, g, true, out_dev);
        if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) dfid_at(rv(SPORCO_AMD_VAR_Y), out_dev, &p);
        read_out(out_dev, out_host);
        // An image whose search has not ended: the apply pass did nothing.  Further passes, until it has.
        double tmp[kOutSlots];
        const int yslots[7] = {SPORCO_AMD_OUT_R2, SPORCO_AMD_OUT_S2, SPORCO_AMD_OUT_AX2, SPORCO_AMD_OUT_Y2,
                               SPORCO_AMD_OUT_U2, SPORCO_AMD_OUT_CGIT, SPORCO_AMD_OUT_CGN};
        const int cslots[3] = {SPORCO_AMD_OUT_L1, SPORCO_AMD_OUT_CNSTR, SPORCO_AMD_OUT_RGRX};
        for (int round = 0; out_host[SPORCO_AMD_OUT_CGIT] != 0.0; ++round) {
            SA_REQUIRE(round < 64, "projl1_iter: the threshold search did not end");
            SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
            projl1_ystep_launches(p, gamma, g, false, out_dev);
            if (want && at_y) projl1_cnstr_launches(rv(SPORCO_AMD_VAR_Y), gamma, g, true, out_dev);
            if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) dfid_at(rv(SPORCO_AMD_VAR_Y), out_dev, &p);
            read_out(out_dev, tmp);
            for (int s : yslots) out_host[s] = tmp[s];
            if (want && at_y)
                for (int s : cslots) out_host[s] = tmp[s];
            if ((p.flags & F_OBJ) && (p.flags & F_FEVAL_Y)) out_host[SPORCO_AMD_OUT_DFID] = tmp[SPORCO_AMD_OUT_DFID];
        }
        for (int round = 0; want && out_host[SPORCO_AMD_OUT_CNSTR] != 0.0; ++round) {
            SA_REQUIRE(round < 64, "projl1_iter: the threshold search did not end");
            SA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * kOutSlots, st));
            projl1_cnstr_launches(at_y ? rv(SPORCO_AMD_VAR_Y) : rv(SPORCO_AMD_VAR_X), gamma, g, false, out_dev);
            read_out(out_dev, tmp);
            for (int s : cslots) out_host[s] = tmp[s];
        }
    }
