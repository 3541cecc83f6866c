// pcs_handle.inc — what the handles share; included after pcs_common.inc.  Plain structs and free functions.  DevBuf and open_device serve
// every handle, the two engine kinds (pcs_engine, pcs_genchain) included; the fence, the timer, the output slots and the checks of
// set_observations serve the batched handles (pcs_triangulator.inc, pcs_pnp.inc, pcs_intrinsics.inc, pcs_rig.inc, pcs_stats.inc).  What
// they guarantee is in DESIGN.md, "Batched handles".

// One growable device buffer: a pointer and its capacity in elements.
struct DevBuf {
    void *p = nullptr;
    int64_t cap = 0;
    template <class T> T *as() const { return static_cast<T *>(p); }
    bool grows(int64_t need) const { return need > cap; }
    hipError_t alloc(int64_t need, size_t elem_bytes) {   // an EMPTY buffer only; it stays empty on failure (create: the caller words the error)
        const hipError_t e = hipMalloc(&p, elem_bytes * (size_t)need);
        if (e == hipSuccess) cap = need;
        return e;
    }
    int grow(int64_t need, size_t elem_bytes) {   // free, then malloc: the contents are not kept
        if (!grows(need)) return PCS_OK;
        if (p) HIPCHK(hipFree(p));
        p = nullptr, cap = 0;
        HIPCHK(alloc(need, elem_bytes));
        return PCS_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

// The Gaussian parameter prior of an engine handle (pcs_set_prior / pcs_genchain_set_prior; kernels: csrc/ba_prior.hpp): the entries with
// weight > 0 only — index into the parameter string, mean, 1 / sigma — on the device, so that a prior on a few intrinsics of a
// million-point problem costs nothing per point; plus the partial cost sums of a list longer than one workgroup's share.  It belongs to
// the HANDLE, not to its detection table: a new table keeps it.  The host keeps the arrays as they were given (pcs_get_prior).
struct PriorStore {
    DevBuf data, partial;                    // data: [index (int64) | mean | 1 / sigma], n words of 8 bytes each: ONE upload per pcs_set_prior
    int64_t n = 0;                           // entries with weight > 0; 0 = no prior
    std::vector<double> h_mean, h_w;         // the n_params values of the last accepted call (empty: none)
    bool active() const { return n > 0; }
    int64_t workgroups() const { return (n + PRIOR_PER_WG - 1) / PRIOR_PER_WG; }
    const int64_t *idx() const { return data.as<const int64_t>(); }
    const double *mean() const { return data.as<const double>() + n; }
    const double *w() const { return data.as<const double>() + 2 * n; }
    // "no prior"; the device buffers stay for the next one (a solve sets and clears its prior: no allocation per solve), and whatever
    // is still queued keeps reading what it was given
    void clear() {
        n = 0;
        h_mean.clear(), h_w.clear();
    }
    void release() {
        data.release(), partial.release();
        clear();
    }
    // everything is checked before anything changes: a refused call leaves the previous prior in force
    static int check(const char *who, const double *mean_in, const double *inv_sigma, int64_t n_in, int64_t n_params) {
        if (!inv_sigma) return PCS_OK;
        if (!mean_in) return fail(PCS_ERR_ARG, "%s: inv_sigma without mean", who);
        if (n_in != n_params) return fail(PCS_ERR_ARG, "%s: %lld values for a parameter string of %lld", who, (long long)n_in, (long long)n_params);
        for (int64_t i = 0; i < n_in; ++i) {
            if (!std::isfinite(inv_sigma[i]) || !(inv_sigma[i] >= 0.0))
                return fail(PCS_ERR_ARG, "%s: inv_sigma %lld = %g must be finite and >= 0", who, (long long)i, inv_sigma[i]);
            if (inv_sigma[i] > 0.0 && !std::isfinite(mean_in[i])) return fail(PCS_ERR_ARG, "%s: mean %lld = %g must be finite where inv_sigma > 0", who, (long long)i, mean_in[i]);
        }
        return PCS_OK;
    }
    // does replacing the prior by these values write device memory that a queued launch may still read?  (the caller then waits first)
    bool set_writes_device(const double *inv_sigma) const { return inv_sigma && data.p; }
    // checked values (or inv_sigma = NULL: none).  A failed allocation or copy leaves "no prior".
    int set(const double *mean_in, const double *inv_sigma, int64_t n_params) {
        clear();
        if (!inv_sigma) return PCS_OK;
        int64_t m = 0;
        for (int64_t i = 0; i < n_params; ++i) m += inv_sigma[i] > 0.0 ? 1 : 0;
        std::vector<uint64_t> words(3 * (size_t)m);
        int64_t k = 0;
        for (int64_t i = 0; i < n_params; ++i)
            if (inv_sigma[i] > 0.0) {
                words[k] = (uint64_t)i;
                memcpy(&words[m + k], &mean_in[i], sizeof(double));
                memcpy(&words[2 * m + k], &inv_sigma[i], sizeof(double));
                ++k;
            }
        if (m > 0) {
            if (const int rc = data.grow(3 * m, sizeof(uint64_t))) return rc;
            if (m > PRIOR_PER_WG)
                if (const int rc = partial.grow((m + PRIOR_PER_WG - 1) / PRIOR_PER_WG, sizeof(double))) return rc;
            const hipError_t e = hipMemcpy(data.p, words.data(), sizeof(uint64_t) * words.size(), hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(PCS_ERR_HIP, "uploading the parameter prior failed: %s", hipGetErrorString(e));
        }
        h_mean.assign(mean_in, mean_in + n_params), h_w.assign(inv_sigma, inv_sigma + n_params);
        n = m;
        return PCS_OK;
    }
    int get(const char *who, double *mean_out, double *inv_sigma, int64_t capacity, int64_t *n_out) const {
        if (capacity < 0 || (!mean_out && !inv_sigma && !n_out)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
        const int64_t have = (int64_t)h_w.size();
        if (n_out) *n_out = have;
        const int64_t m = std::min(have, capacity);
        if (mean_out && m > 0) memcpy(mean_out, h_mean.data(), sizeof(double) * m);
        if (inv_sigma && m > 0) memcpy(inv_sigma, h_w.data(), sizeof(double) * m);
        return PCS_OK;
    }
};

// The box bounds of an engine handle (pcs_set_bounds / pcs_genchain_set_bounds; kernels: csrc/ba_bounds.hpp): lo and hi over the whole
// parameter string on the device (-inf / +inf = none), the effective mask a trial's Schur step reads in place of the caller's, and the
// words a trial leaves behind: alpha, the number of truncated trials, the number of active entries, and (alpha, active entries) of the
// first BOUNDS_LOG_TRIALS trials of the loop.  It belongs to the HANDLE, not to its detection table: a new table keeps it.  The host
// keeps the arrays as they were given (pcs_get_bounds).
struct BoundStore {
    DevBuf pins;                             // n bytes: entries pinned by the last rejected trials (csrc/ba_bounds.hpp)
    DevBuf data, eff, words;                 // data: [lo | hi], 2 n doubles, ONE upload per pcs_set_bounds; eff: n bytes; words: [alpha | truncated trials | active entries (int32) | log]
    int64_t n = 0;                           // n_params while bounds are set; 0 = none
    std::vector<double> h_lo, h_hi;
    static constexpr int64_t WORDS = 3 + 2 * (int64_t)BOUNDS_LOG_TRIALS;
    bool active() const { return n > 0; }
    const double *lo() const { return data.as<const double>(); }
    const double *hi() const { return data.as<const double>() + n; }
    uint8_t *fixed_eff() const { return eff.as<uint8_t>(); }
    uint8_t *pin() const { return pins.as<uint8_t>(); }
    double *alpha() const { return words.as<double>(); }
    double *n_truncated() const { return words.as<double>() + 1; }
    int32_t *n_active() const { return reinterpret_cast<int32_t *>(words.as<double>() + 2); }
    double *log() const { return words.as<double>() + 3; }
    // "no bounds"; the device buffers stay for the next ones (a solve sets and clears its bounds: no allocation per solve)
    void clear() {
        n = 0;
        h_lo.clear(), h_hi.clear();
    }
    void release() {
        data.release(), eff.release(), words.release(), pins.release();
        clear();
    }
    // everything is checked before anything changes: a refused call leaves the previous bounds in force
    static int check(const char *who, const double *lo_in, const double *hi_in, int64_t n_in, int64_t n_params) {
        if (!lo_in && !hi_in) return PCS_OK;
        if (!lo_in || !hi_in) return fail(PCS_ERR_ARG, "%s: lo and hi come together (both NULL: no bounds)", who);
        if (n_in != n_params) return fail(PCS_ERR_ARG, "%s: %lld values for a parameter string of %lld", who, (long long)n_in, (long long)n_params);
        for (int64_t i = 0; i < n_in; ++i) {
            if (lo_in[i] != lo_in[i] || hi_in[i] != hi_in[i]) return fail(PCS_ERR_ARG, "%s: bound %lld is NaN", who, (long long)i);
            if (lo_in[i] > hi_in[i]) return fail(PCS_ERR_ARG, "%s: lo %lld = %g > hi = %g", who, (long long)i, lo_in[i], hi_in[i]);
        }
        return PCS_OK;
    }
    // does replacing the bounds by these values write device memory that a queued launch may still read?  (the caller then waits first)
    bool set_writes_device(const double *lo_in) const { return lo_in && data.p; }
    // checked values (or NULL: none).  A failed allocation or copy leaves "no bounds".
    int set(const double *lo_in, const double *hi_in, int64_t n_params) {
        clear();
        if (!lo_in || n_params <= 0) return PCS_OK;
        if (const int rc = data.grow(2 * n_params, sizeof(double))) return rc;
        if (const int rc = eff.grow(n_params, 1)) return rc;
        if (const int rc = pins.grow(n_params, 1)) return rc;
        if (const int rc = words.grow(WORDS, sizeof(double))) return rc;
        std::vector<double> both(2 * (size_t)n_params);
        memcpy(both.data(), lo_in, sizeof(double) * n_params);
        memcpy(both.data() + n_params, hi_in, sizeof(double) * n_params);
        hipError_t e = hipMemcpy(data.p, both.data(), sizeof(double) * both.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(eff.p, 0, (size_t)n_params);
        if (e == hipSuccess) e = hipMemset(pins.p, 0, (size_t)n_params);
        if (e == hipSuccess) e = hipMemset(words.p, 0, sizeof(double) * WORDS);
        const double one = 1.0;
        if (e == hipSuccess) e = hipMemcpy(words.p, &one, sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(PCS_ERR_HIP, "uploading the parameter bounds failed: %s", hipGetErrorString(e));
        h_lo.assign(lo_in, lo_in + n_params), h_hi.assign(hi_in, hi_in + n_params);
        n = n_params;
        return PCS_OK;
    }
    int get(const char *who, double *lo_out, double *hi_out, int64_t capacity, int64_t *n_out) const {
        if (capacity < 0 || (!lo_out && !hi_out && !n_out)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
        const int64_t have = (int64_t)h_lo.size();
        if (n_out) *n_out = have;
        const int64_t m = std::min(have, capacity);
        if (lo_out && m > 0) memcpy(lo_out, h_lo.data(), sizeof(double) * m);
        if (hi_out && m > 0) memcpy(hi_out, h_hi.data(), sizeof(double) * m);
        return PCS_OK;
    }
    // pcs_bounds_trials: what the decided trials of the last loop left (the caller has synchronised the loop's stream)
    int trials(const char *who, double *alpha_active, int64_t n_trials, int64_t *truncated) const {
        if (n_trials < 0 || (n_trials > 0 && !alpha_active)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
        if (!active()) return fail(PCS_ERR_STATE, "%s: no bounds set", who);
        const int64_t m = std::min<int64_t>(n_trials, BOUNDS_LOG_TRIALS);
        if (m > 0) HIPCHK(hipMemcpy(alpha_active, log(), sizeof(double) * 2 * m, hipMemcpyDeviceToHost));
        for (int64_t k = 2 * m; k < 2 * n_trials; ++k) alpha_active[k] = std::nan("");
        if (truncated) {
            double t = 0.0;
            HIPCHK(hipMemcpy(&t, n_truncated(), sizeof(double), hipMemcpyDeviceToHost));
            *truncated = (int64_t)t;
        }
        return PCS_OK;
    }
};

// Ordering of a handle's runs across streams: `done` is recorded after every run; whatever touches what a run reads or writes next
// waits for it first.  (pcs_engine.hip's flush_done / mark_done are the lazily recording variant of this for the engine.)
struct RunFence {
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;   // compared only, never used as a handle again
    bool have_done = false;
    hipError_t create() { return hipEventCreateWithFlags(&done, hipEventDisableTiming); }
    void destroy() {
        if (done) (void)hipEventDestroy(done);
        done = nullptr, have_done = false;
    }
    hipError_t wait_host() const { return have_done ? hipEventSynchronize(done) : hipSuccess; }
    // Scratch and outputs are shared between runs, so the previous run finishes first.  A call that grows a buffer frees one, and a free
    // needs the host to wait; hipStreamWaitEvent on the legacy stream is avoided, so there the host waits as well.  Another stream waits
    // for the event; the same stream is ordered already.
    hipError_t before_run(hipStream_t s, bool grows) const {
        if (!have_done) return hipSuccess;
        if (grows || s == hipStreamLegacy || done_stream == hipStreamLegacy) return hipEventSynchronize(done);
        return s != done_stream ? hipStreamWaitEvent(s, done, 0) : hipSuccess;
    }
    hipError_t after_run(hipStream_t s) {
        have_done = true, done_stream = s;
        return hipEventRecord(done, s);
    }
};

// Device time of the last run: two events and whether they were ever recorded.
struct KernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool timed = false;
    hipError_t create() {
        const hipError_t e = hipEventCreate(&e0);
        return e == hipSuccess ? hipEventCreate(&e1) : e;
    }
    void destroy() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = nullptr;
    }
};

static int timer_ms(const char *who, KernelTimer *t, float *kernel_ms, const char *nothing_yet) {
    if (!t || !kernel_ms) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!t->timed) return fail(PCS_ERR_STATE, "%s: %s", who, nothing_yet);
    HIPCHK(hipEventSynchronize(t->e1));
    HIPCHK(hipEventElapsedTime(kernel_ms, t->e0, t->e1));
    return PCS_OK;
}

// The device, the handle's own stream and the fence of its runs.
struct HandleCore {
    int device = 0;
    hipStream_t stream = nullptr;
    RunFence fence;
    hipError_t create(int dev) {
        device = dev;
        const hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        return e == hipSuccess ? fence.create() : e;
    }
    // a run queued on ANY stream may still read what the caller is about to overwrite, free or fetch
    hipError_t quiesce() const {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = fence.wait_host();
        if (e == hipSuccess && stream) e = hipStreamSynchronize(stream);
        return e;
    }
    hipStream_t stream_or(void *caller) const { return caller ? (hipStream_t)caller : stream; }
    void destroy(std::initializer_list<DevBuf *> bufs, std::initializer_list<KernelTimer *> timers) {
        (void)quiesce();
        for (DevBuf *b : bufs) b->release();
        for (KernelTimer *t : timers) t->destroy();
        fence.destroy();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The two engine kinds and the block check word both refusals at more length than the batched handles: `no_fallback` says what has no CPU
// fallback, `show_range` puts the device and the range into the second message.
static int open_device(const char *who, int device, const char *no_fallback = "no CPU fallback", bool show_range = false) {
    const int ndev = pcs_device_count();
    if (ndev <= 0) return fail(PCS_ERR_NODEVICE, "%s: no HIP device visible (%s)", who, no_fallback);
    if (device < 0 || device >= ndev)
        return show_range ? fail(PCS_ERR_ARG, "%s: device %d out of range [0,%d)", who, device, ndev) : fail(PCS_ERR_ARG, "%s: device out of range", who);
    HIPCHK(hipSetDevice(device));
    return PCS_OK;
}

// `rest_ok` / `rest`: the caller's own options and their wording, so that one message names every constraint
static int check_lm_options(const char *who, int max_iter, double ftol, double xtol, double gtol, bool rest_ok, const char *rest) {
    if (!rest_ok || max_iter < 0 || !(ftol >= 0.0 && ftol < INFINITY) || !(xtol >= 0.0 && xtol < INFINITY) || !(gtol >= 0.0 && gtol < INFINITY))
        return fail(PCS_ERR_ARG, "%s: bad options (max_iter >= 0, finite tolerances >= 0, %s)", who, rest);
    return PCS_OK;
}

// The loss of a batched handle (pcs_rigpose_set_loss, pcs_tri_set_refine_loss): the checks of pcs_set_loss.  Nothing changes on a refusal.
struct HandleLoss {
    int kind = PCS_LOSS_LINEAR;
    double f_scale = 1.0;
    GroupLoss args() const { return {kind, 1.0 / f_scale, f_scale * f_scale}; }
};

static int set_handle_loss(const char *who, HandleLoss *l, int kind, double f_scale) {
    if (!l) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (kind < PCS_LOSS_LINEAR || kind > PCS_LOSS_ARCTAN) return fail(PCS_ERR_ARG, "%s: kind %d not in [0, 4] (linear, huber, soft_l1, cauchy, arctan)", who, kind);
    if (!std::isfinite(f_scale) || !(f_scale > 0.0)) return fail(PCS_ERR_ARG, "%s: f_scale must be finite and > 0 (got %g)", who, f_scale);
    l->kind = kind;
    l->f_scale = f_scale;
    return PCS_OK;
}

static int get_handle_loss(const char *who, const HandleLoss *l, int *kind, double *f_scale) {
    if (!l) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (kind) *kind = l->kind;
    if (f_scale) *f_scale = l->f_scale;
    return PCS_OK;
}

// The grouped table of a set_observations call: start_inds runs from 0 to n_obs and never decreases, and every observation's key lies
// in [0, n_keys).  `group_ok(j)` checks the handle's own per-group columns (0, or the code of its refusal);
// it runs in group order right behind group j's start index, so that the first bad GROUP decides the refusal, ahead of any bad key.
template <class GroupOk>
static int check_grouped_observations(const char *who, int64_t n_obs, const int32_t *key, int64_t n_keys, int64_t n_groups, const int64_t *start_inds,
                                      GroupOk group_ok) {
    if (start_inds[0] != 0 || start_inds[n_groups] != n_obs) return fail(PCS_ERR_ARG, "%s: start_inds must run from 0 to n_obs", who);
    for (int64_t j = 0; j < n_groups; ++j) {
        if (start_inds[j + 1] < start_inds[j]) return fail(PCS_ERR_ARG, "%s: start_inds must be non-decreasing", who);
        if (const int rc = group_ok(j)) return rc;
    }
    for (int64_t r = 0; r < n_obs; ++r)
        if (key[r] < 0 || key[r] >= n_keys) return fail(PCS_ERR_RANGE, "observation %lld has key %d outside [0,%lld)", (long long)r, key[r], (long long)n_keys);
    return PCS_OK;
}

// a group's camera / image column
static int check_group_entity(const char *group, int64_t j, const char *what, int32_t v, int64_t count) {
    if (v < 0 || v >= count) return fail(PCS_ERR_RANGE, "%s %lld has %s %d outside [0,%lld)", group, (long long)j, what, v, (long long)count);
    return PCS_OK;
}

// A host array into a buffer of fixed size (allocated at create): a run queued on any stream may still read it, so the handle is quiesced first
static int set_fixed_array(const HandleCore &c, DevBuf &buf, const void *src, size_t bytes) {
    HIPCHK(c.quiesce());
    HIPCHK(hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
    return PCS_OK;
}

// Host arrays copied into handle-owned buffers (set_observations): every allocation first, then the copies on the handle's stream, then
// a wait, so that the caller may reuse its arrays.  A buffer is never empty: at least one element is allocated.
struct HostArray {
    DevBuf &buf;
    const void *src;
    int64_t count;
    size_t elem_bytes;
};

static int upload_host_arrays(const HandleCore &c, const HostArray *a, int n) {
    for (int i = 0; i < n; ++i)
        if (const int rc = a[i].buf.grow(std::max<int64_t>(1, a[i].count), a[i].elem_bytes)) return rc;
    for (int i = 0; i < n; ++i)
        if (a[i].count) HIPCHK(hipMemcpyAsync(a[i].buf.p, a[i].src, a[i].elem_bytes * (size_t)a[i].count, hipMemcpyHostToDevice, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return PCS_OK;
}

// One output of a run: it goes to the caller's device buffer or, when the caller passed none, to a handle-owned one (PCS_*_OUT_* bit
// set in `owned`).  Fetching uses the same slot with `ptr` the caller's HOST array.
struct OutSlot {
    int bit;
    DevBuf &buf;
    void *ptr;       // run: in, the caller's device buffer or NULL; after grow_owned_slots, where the run writes.  fetch: the host array or NULL
    int64_t count;   // elements the run writes / the fetch copies (at least one is allocated)
    size_t elem_bytes;
    template <class T> T *as() const { return static_cast<T *>(ptr); }
};

static int owned_slots(const OutSlot *sl, int n, bool *grows) {
    int owned = 0;
    for (int i = 0; i < n; ++i)
        if (!sl[i].ptr) {
            owned |= sl[i].bit;
            *grows = *grows || sl[i].buf.grows(sl[i].count);   // the one element of an empty output replaces nothing: no wait for it
        }
    return owned;
}

// after the fence, before the first enqueue: nothing is queued by a call that fails in an allocation
static int grow_owned_slots(OutSlot *sl, int n) {
    for (int i = 0; i < n; ++i)
        if (!sl[i].ptr) {
            if (const int rc = sl[i].buf.grow(std::max<int64_t>(1, sl[i].count), sl[i].elem_bytes)) return rc;
            sl[i].ptr = sl[i].buf.p;
        }
    return PCS_OK;
}

// The handle-owned outputs of the last run to the host arrays of the slots that have one; refused when the run wrote one of them
// elsewhere.  `ran`: false for an empty problem, which has nothing to copy.
static int fetch_slots(const HandleCore &c, const OutSlot *sl, int n, int owned, bool ran, const char *who, const char *refusal) {
    int want = 0;
    for (int i = 0; i < n; ++i) want |= sl[i].ptr ? sl[i].bit : 0;
    if (want & ~owned) return fail(PCS_ERR_STATE, "%s: %s", who, refusal);
    if (!ran) return PCS_OK;
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(c.fence.wait_host());   // the run may have been queued on a caller stream
    for (int i = 0; i < n; ++i)
        if (sl[i].ptr && sl[i].count)
            HIPCHK(hipMemcpyAsync(sl[i].ptr, sl[i].buf.p, sl[i].elem_bytes * (size_t)sl[i].count, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipStreamSynchronize(c.stream));
    return PCS_OK;
}

// The (n_groups, 2) costs of a run, always handle-owned.  A robust run writes them itself.  A LINEAR run stays what it was before the
// handles knew a loss — no buffer, no launch: its costs are derived when they are asked for, 0.5 n rms^2 from the RMS the run wrote
// (group_cost_from_rms_kernel), read where the run wrote it.
struct LinearCosts {
    const double *rms = nullptr;      // the (n_groups, 2) RMS of the last linear run: handle-owned or the caller's device buffer
    const int64_t *start = nullptr;   // its start indices
    bool pending = false;             // not derived yet
};

static int fetch_costs(const HandleCore &c, DevBuf &cost, LinearCosts &lin, double *host, int64_t n_groups, const char *who) {
    if (lin.pending && n_groups) {
        HIPCHK(hipSetDevice(c.device));
        HIPCHK(c.fence.wait_host());   // the run first (it may be queued on a caller stream); growing frees, which needs the host to wait anyway
        if (const int rc = cost.grow(n_groups, 2 * sizeof(double))) return rc;
        hipLaunchKernelGGL(group_cost_from_rms_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, c.stream, lin.rms, lin.start, n_groups,
                           cost.as<double>());
        HIPCHK(hipGetLastError());
        lin.pending = false;
    }
    const OutSlot out{1, cost, host, n_groups, 2 * sizeof(double)};
    return fetch_slots(c, &out, 1, 1, n_groups != 0, who, "");   // copies on the same stream, behind the kernel
}

// The visiting order of n groups given by their start indices: groups of like size side by side, so that a wave does not mix small and
// large ones (counts above 255 share a bucket).  d_hist: 512 int32; queued on the run's own stream (the start indices may have been
// produced there).
constexpr int64_t GROUP_ORDER_HIST = 512;
static int enqueue_group_order(const int64_t *d_start, int64_t n, int32_t *d_hist, int32_t *d_order, hipStream_t s) {
    HIPCHK(hipMemsetAsync(d_hist, 0, sizeof(int32_t) * GROUP_ORDER_HIST, s));
    const dim3 pg((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(tri_order_count_kernel, pg, dim3(256), 0, s, d_start, n, d_hist);
    hipLaunchKernelGGL(tri_order_scan_kernel, dim3(1), dim3(256), 0, s, d_hist);
    hipLaunchKernelGGL(tri_order_scatter_kernel, pg, dim3(256), 0, s, d_start, n, d_hist, d_order);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}

// Behind the select kernel of a consensus stage with G lanes per problem: c_start = the exclusive scan of the inlier counts cinfo[4 j],
// then the flagged rows of both columns of the table to (c_col, c_uv) in their order.  The caller checks hipGetLastError.
template <int G>
static void enqueue_compact_flagged(const int32_t *col, const double2 *uv, const int64_t *start, const uint8_t *flag, const int32_t *cinfo, int64_t n,
                                    int64_t *c_start, int32_t *c_col, double2 *c_uv, hipStream_t s) {
    hipLaunchKernelGGL(cons_count_scan_kernel, dim3(1), dim3(CONS_SCAN_THREADS), 0, s, cinfo, n, c_start);
    hipLaunchKernelGGL((cons_compact_kernel<G>), dim3((unsigned)((n * G + 255) / 256)), dim3(256), 0, s, col, uv, start, flag, (const int64_t *)c_start, n,
                       c_col, c_uv);
}
