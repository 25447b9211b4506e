// api_placement.inc -- member functions of template Csc<T> (csc_api.hip includes this file INSIDE the
// class body): where the X-sized arrays that a kernel WRITES AT THE SAME TIME lie in HBM.
//
// What was measured (tools/ubench/place_probe.hip, profiles/r05_placement_notes.md): on the MI355X two
// arrays that take streaming stores concurrently share ~4.7 TB/s when their physical memory lies in
// the same region of the device memory and get ~6.3 TB/s when it lies in different ones; reads do
// not care.  Regions are runs of physical memory several GiB long (4 ... 64 GiB in allocation
// order, different from box to box); virtual addresses and distances say nothing about them.  The
// emitting row epilogue (csc_rows.h) writes the spectrum T' and the iterate V' at once: 1.47 ms per
// launch at the headline shape when T and V' lie in different regions, 1.77 ms when they share one
// -- the three "levels" of round 4 (both V buffers apart from T, one, none).
//
// What the library does about it: a region cannot be asked for, but it can be measured.  A buffer that
// will be written together with others is taken from a few candidate allocations, each timed against
// the arrays it must keep clear of with launch_place_probe (both rewritten in place at once -- nothing
// is modified) relative to the same probe on the two halves of one array (same region by
// construction); rejected candidates wait in `spare_big` for the next large allocation of the
// handle.  Only for arrays of 256 MiB ... 4 GiB on the register-resident path, at most 12
// candidates / 24 GiB / 0.4 s per decision; SPORCO_AMD_PLACEMENT=0 switches it off.
    struct PlaceRec {
        const char *role;
        size_t bytes;
        int tried;
        double ref_gbps, first_ratio, chosen_ratio;
        double ms;
    };
    std::vector<PlaceRec> place_log;
    std::vector<std::pair<void *, size_t>> spare_big;   // allocated, unused: (pointer handed out by big_alloc, bytes)
    std::vector<const void *> spare_vs;                 // ... and the array each was last rejected against
    hipEvent_t place_ev[2] = {nullptr, nullptr};
    // probe rate / same-region rate: clear of each other from here on.  Measured: same region
    // 0.92 ... 1.00, different regions 1.06 ... 1.17 (round 6, three allocation histories: buffers
    // chosen at 1.06 ... 1.11 all run the emitting epilogue at 1.505 ... 1.547 ms in BOTH ping-pong
    // directions -- bench.py `roofline.per_direction_ms` -- and a search that insists on 1.085 spends
    // its whole candidate budget without finding better).
    static constexpr double kPlaceClear = 1.05;
    static constexpr int kPlaceMaxCandidates = 12;                 // per decision, and at most
    static constexpr size_t kPlaceMaxBytes = (size_t)24 << 30;     // ... this much candidate memory
    static constexpr size_t kPlaceMaxArray = (size_t)4 << 30;      // arrays beyond this: placed as they come
    static constexpr size_t kPlaceMaxHeld = (size_t)96 << 30;      // candidates held at once, all decisions
    static constexpr double kPlaceMaxMs = 400.0;                   // ... and this long
    static constexpr size_t kPlaceMinBytes = (size_t)256 << 20;

    bool placement_on(size_t bytes) const {
        if (sw.placement_force) return !sw.placement_off && rows_ok && (fused || fused_slabs);
        // (arrays of many GiB straddle regions whatever is done -- runs are 4 ... 64 GiB long -- and a
        // candidate of that size costs hundreds of milliseconds: placed as they come)
        return !sw.placement_off && bytes >= kPlaceMinBytes && bytes <= kPlaceMaxArray && rows_ok &&
               (fused || fused_slabs);
    }

    // GB/s of stores when a and b (ba, bb bytes) are rewritten in place at the same time; arrays
    // beyond 512 MiB are sampled in four windows of 128 MiB spread evenly over each (regions are runs
    // of GiB: four samples say which ones an array lies in, at an eighth of the traffic of a 2 GiB pair)
    double place_rate(void *a, size_t ba, void *b, size_t bb) {
        if (!place_ev[0]) {
            SA_HIP(hipEventCreate(&place_ev[0]));
            SA_HIP(hipEventCreate(&place_ev[1]));
        }
        const int64_t na = (int64_t)(ba / 16), nb = (int64_t)(bb / 16), cap = (int64_t)1 << 25;
        int64_t n = std::min(na, nb), win = n, sa = 0, sb = 0;
        if (n > cap) {
            win = cap / 4;
            n = cap;
            sa = (na - win) / 3;
            sb = (nb - win) / 3;
        }
        // One measurement = four launches with b walked from 0, 1/4, 1/2, 3/4 of its length on: a
        // kernel's write streams are not in step (the epilogue writes T' all over the spectrum
        // buffer while V' advances row by row), and an array may be made of physical blocks from
        // more than one region -- every part of a meets every part of b.  The better of two
        // measurements after a warm-up launch (the first launches after host-side set-up run on a
        // device that is still raising its clocks).
        launch_place_probe(st, a, b, n, win, sa, sb, false, false, 0);
        float best = 0.f;
        for (int i = 0; i < 2; ++i) {
            SA_HIP(hipEventRecord(place_ev[0], st));
            for (int k = 0; k < 4; ++k) launch_place_probe(st, a, b, n, win, sa, sb, false, false, k * (n / 4));
            SA_HIP(hipEventRecord(place_ev[1], st));
            SA_HIP(hipEventSynchronize(place_ev[1]));
            float ms = 0.f;
            SA_HIP(hipEventElapsedTime(&ms, place_ev[0], place_ev[1]));
            if (ms > 0.f && (best == 0.f || ms < best)) best = ms;
        }
        return best > 0.f ? 4.0 * 2.0 * (double)n * 16.0 / ((double)best * 1e6) : 0.0;
    }
    // the same-region reference: the two halves of one array
    double place_ref(void *a, size_t bytes) {
        const size_t half = (bytes / 2) & ~(size_t)4095;
        return place_rate(a, half, static_cast<char *>(a) + half, half);
    }

    // A buffer of `bytes` bytes that is clear of every array in `avoid` (pointer, bytes), or the best
    // of the candidates tried.  Contents undefined.
    void *place_alloc(size_t bytes, const std::vector<std::pair<void *, size_t>> &avoid, const char *role,
                      double *ratio_out = nullptr) {
        void *p = nullptr;
        if (ratio_out) *ratio_out = 0.0;
        if (!placement_on(bytes) || avoid.size() == 0) {
            big_alloc(&p, bytes);
            return p;
        }
        const auto t0 = std::chrono::steady_clock::now();
        // (the reference is taken again beside every candidate and the highest value counts: see
        // place_rate on clocks)
        double ref = place_ref(avoid.begin()->first, avoid.begin()->second);
        struct Cand {
            void *p;
            size_t bytes;
            double rate, ratio;
        };
        std::vector<Cand> tried;
        auto score = [&](void *c, size_t cb) {
            double r = 1e30;
            for (const auto &av : avoid) r = std::min(r, place_rate(av.first, av.second, c, cb));
            ref = std::max(ref, place_ref(avoid.begin()->first, avoid.begin()->second));
            return r;
        };
        int best = -1;
        const void *const vs = avoid.begin()->first;
        auto take = [&](Cand c) {
            c.rate = score(c.p, bytes);
            tried.push_back(c);
            if (best < 0 || c.rate > tried[best].rate) best = (int)tried.size() - 1;
            return c.rate / ref >= kPlaceClear;
        };
        bool found = false;
        // 1. what earlier decisions of this handle set aside -- except what was already rejected
        //    against the same array (held, not freed: freeing a rejected candidate hands the next
        //    hipMalloc the same memory again, and a search would never leave a long region)
        for (size_t i = 0; i < spare_big.size() && !found;) {
            if (spare_big[i].second < bytes || spare_big[i].second > bytes + bytes / 8 || spare_vs[i] == vs) {
                ++i;
                continue;
            }
            const Cand c{spare_big[i].first, spare_big[i].second, 0.0, 0.0};
            spare_big.erase(spare_big.begin() + i);
            spare_vs.erase(spare_vs.begin() + i);
            found = take(c);
        }
        // 2. fresh allocations, while memory and time are plentiful
        const int max_cand = sw.placement_force ? 3 : (int)std::min<size_t>(kPlaceMaxCandidates, kPlaceMaxBytes / bytes);
        const auto t1 = std::chrono::steady_clock::now();
        for (int round = 0; round < max_cand && !found; ++round) {
            if (round > 0 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count() > kPlaceMaxMs)
                break;
            size_t held = 0;
            for (const auto &sp : spare_big) held += sp.second;
            for (const auto &c : tried) held += c.bytes;
            // (never more than half of what is free now in candidates of this handle -- another
            // process on the device must be able to allocate while a search runs -- and never the
            // last six arrays' worth)
            size_t free_b = 0, total_b = 0;
            if (held + bytes > kPlaceMaxHeld || hipMemGetInfo(&free_b, &total_b) != hipSuccess ||
                free_b < 6 * bytes || held + bytes > (free_b + held) / 2)
                break;
            Cand c{nullptr, bytes, 0.0, 0.0};
            try {
                big_alloc_fresh(&c.p, bytes);
            } catch (const Error &) {
                (void)hipGetLastError();
                break;
            }
            found = take(c);
        }
        if (best < 0) {
            big_alloc(&p, bytes);
            return p;
        }
        p = tried[best].p;
        for (auto &c : tried) c.ratio = c.rate / ref;
        for (int i = 0; i < (int)tried.size(); ++i)
            if (i != best) {
                spare_big.emplace_back(tried[i].p, tried[i].bytes);
                spare_vs.push_back(vs);
            }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        place_log.push_back(PlaceRec{role, bytes, (int)tried.size(), ref, tried[0].ratio, tried[best].ratio, ms});
        if (ratio_out) *ratio_out = tried[best].ratio;
        return p;
    }
    // A state variable clear of others (variable ids; the ones that do not exist yet are ignored): it is
    // allocated that way if it does not exist, and moved -- one device copy -- if it exists and shares
    // a region with any of them.
    void place_var(int var, std::initializer_list<int> avoid_vars, const char *role) {
        const size_t nb = var_alloc_bytes(var);
        std::vector<std::pair<void *, size_t>> av;
        for (int v : avoid_vars)
            if (vars[v] && v != var) av.emplace_back(vars[v], var_alloc_bytes(v));
        if (!placement_on(nb) || av.empty()) {
            (void)var_ptr(var);
            return;
        }
        if (!vars[var]) {
            vars[var] = place_alloc(nb, av, role);
            SA_HIP(hipMemsetAsync(vars[var], 0, nb, st));
            return;
        }
        double ref = place_ref(av[0].first, av[0].second), r = 1e30;
        for (const auto &a : av) r = std::min(r, place_rate(a.first, a.second, vars[var], nb));
        ref = std::max(ref, place_ref(av[0].first, av[0].second));
        r /= ref;
        if (r >= kPlaceClear) return;
        double rn = 0.0;
        void *np = place_alloc(nb, av, role, &rn);
        if (rn <= r) {   // nothing better found: stay
            spare_big.emplace_back(np, nb);
            spare_vs.push_back(av[0].first);
            return;
        }
        SA_HIP(hipMemcpyAsync(np, vars[var], nb, hipMemcpyDeviceToDevice, st));
        SA_HIP(hipStreamSynchronize(st));
        spare_big.emplace_back(vars[var], nb);
        spare_vs.push_back(av[0].first);
        vars[var] = np;
    }
    void place_release_spares() {
        for (auto &s : spare_big) big_free(s.first);
        spare_big.clear();
        spare_vs.clear();
    }
    // one line of JSON per decision (sporco_amd_csc_placement_report)
    std::string placement_report() const {
        std::string out = "[";
        char buf[256];
        for (size_t i = 0; i < place_log.size(); ++i) {
            const PlaceRec &r = place_log[i];
            std::snprintf(buf, sizeof buf,
                          "%s{\"role\": \"%s\", \"bytes\": %zu, \"candidates\": %d, \"same_region_GBps\": %.0f, "
                          "\"first_ratio\": %.3f, \"chosen_ratio\": %.3f, \"clear\": %s, \"ms\": %.1f}",
                          i ? ", " : "", r.role, r.bytes, r.tried, r.ref_gbps, r.first_ratio, r.chosen_ratio,
                          r.chosen_ratio >= kPlaceClear ? "true" : "false", r.ms);
            out += buf;
        }
        return out + "]";
    }
