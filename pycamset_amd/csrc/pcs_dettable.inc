// pcs_dettable.inc — the detection table both engine kinds (pcs_engine, pcs_genchain) hold; included after pcs_handle.inc.  DetStore owns the
// host index columns and the device form the kernels read as a DetTable (csrc/ba_device.hpp): one cam | image | key word per detection
// when the widths fit 32 bits, else three int32 arrays; plus the measurements.  Parsing, the range check, the widths and the packing
// are host-only and run without a device (tools/probes/dettable_host_check.hip).

struct DetColumns {
    std::vector<int32_t> cam, img, key;
};

// the entity counts the indices are checked against; no_img: the table has no image column (the free chain)
struct DetCounts {
    int64_t cams = 0, imgs = 0, keys = 0;
    bool no_img = false;
};

static int det_row_in_range(int64_t i, int32_t c, int32_t im, int32_t k, const DetCounts &m) {
    // an out-of-range index would be an out-of-bounds slab read on the device
    if (c < 0 || c >= m.cams || k < 0 || k >= m.keys || (!m.no_img && (im < 0 || im >= m.imgs)))
        return fail(PCS_ERR_RANGE, "detection %lld = (cam %d, im %d, key %d) outside (%lld, %lld, %lld)", (long long)i, c, im, k, (long long)m.cams,
                    (long long)m.imgs, (long long)m.keys);
    return PCS_OK;
}

static int det_check_range(const DetColumns &c, const DetCounts &m) {
    for (size_t i = 0; i < c.cam.size(); ++i)
        if (const int rc = det_row_in_range((int64_t)i, c.cam[i], c.img[i], c.key[i], m)) return rc;
    return PCS_OK;
}

// (N, 5) doubles -> index columns + (N, 2) measurements.  `row_counts`: check every row's range right behind its parse, so that the
// first bad ROW decides the refusal (generated chains); NULL: parse only (the engine checks the range of the whole table afterwards).
static int det_parse(const double *det5, int64_t n, DetColumns &c, std::vector<double> &uv, const DetCounts *row_counts = nullptr) {
    c.cam.resize(n), c.img.resize(n), c.key.resize(n), uv.resize(2 * n);
    for (int64_t i = 0; i < n; ++i) {
        for (int j = 0; j < 3; ++j)   // NaN / huge values have no int32 image: refuse instead of casting
            if (!(det5[5 * i + j] > -1.0 && det5[5 * i + j] < 2147483648.0))
                return fail(PCS_ERR_RANGE, "detection %lld: index column %d = %g is not an index", (long long)i, j, det5[5 * i + j]);
        c.cam[i] = (int32_t)det5[5 * i + 0];   // int() cast like afb:214 / afb:375
        c.img[i] = (int32_t)det5[5 * i + 1];
        c.key[i] = (int32_t)det5[5 * i + 2];
        if (row_counts)
            if (const int rc = det_row_in_range(i, c.cam[i], c.img[i], c.key[i], *row_counts)) return rc;
        uv[2 * i] = det5[5 * i + 3];
        uv[2 * i + 1] = det5[5 * i + 4];
    }
    return PCS_OK;
}

// index word: cam | image | key bit fields when they fit 32 bits (12 -> 4 bytes per detection), else three arrays
struct DetWidths {
    int key_bits = 0, img_bits = 0;
    bool packs = false;
};

static int det_bits_for(int64_t count) {
    int b = 0;
    while (((int64_t)1 << b) < count) ++b;
    return b;
}

static DetWidths det_widths(const DetCounts &m) {
    DetWidths w;
    w.key_bits = det_bits_for(m.keys);
    w.img_bits = m.no_img ? 0 : det_bits_for(m.imgs);   // no image column: its values are not range-checked and take no bits
    w.packs = w.key_bits + w.img_bits + det_bits_for(m.cams) <= 32 && w.key_bits + w.img_bits <= 31;
    return w;
}

static std::vector<uint32_t> det_pack(const DetColumns &c, const DetWidths &w) {
    std::vector<uint32_t> word(c.cam.size());
    for (size_t i = 0; i < word.size(); ++i)
        word[i] = ((uint32_t)c.cam[i] << (w.key_bits + w.img_bits)) | ((w.img_bits ? (uint32_t)c.img[i] : 0u) << w.key_bits) | (uint32_t)c.key[i];
    return word;
}

struct DetStore {
    DetColumns h;                   // host copies of the index columns (visiting orders, CSR structure, segment tables)
    DevBuf packed, cam, img, key;   // the packed word, or the three arrays
    DevBuf uv;                      // float or double measurements
    DevBuf w;                       // noise weights, 1 / sigma per detection in table order (double), or empty = none (pcs_set_weights)
    int key_bits = 0, img_bits = 0;
    bool uv_f32 = false;
    int64_t n = 0;                  // 0 = "no detections set"

    DetTable table() const {
        DetTable t{};
        t.packed = packed.as<const uint32_t>();
        t.cam = cam.as<const int32_t>(); t.img = img.as<const int32_t>(); t.key = key.as<const int32_t>();
        t.uv = uv.p;
        t.key_bits = key_bits; t.img_bits = img_bits;
        t.uv_f32 = uv_f32;
        return t;
    }

    void release() {
        for (DevBuf *b : {&packed, &cam, &img, &key, &uv, &w}) b->release();
        h = DetColumns{};
        n = 0;
    }

    // The checked columns `c` (taken over) and their measurements become the table.  The caller has waited for everything that reads the
    // old one.  pack: use the word when the widths allow.  n is set last: a failed allocation or copy leaves "no detections set".
    int upload(DetColumns &c, const double *uv_host, const DetCounts &m, bool pack, bool f32) {
        release();
        const int64_t count = (int64_t)c.cam.size();
        h.cam.swap(c.cam), h.img.swap(c.img), h.key.swap(c.key);
        if (count == 0) return PCS_OK;
        const DetWidths w = det_widths(m);
        key_bits = w.key_bits, img_bits = w.img_bits, uv_f32 = f32;
        if (pack && w.packs) {
            const std::vector<uint32_t> word = det_pack(h, w);
            if (const int rc = packed.grow(count, sizeof(uint32_t))) return rc;
            HIPCHK(hipMemcpy(packed.p, word.data(), sizeof(uint32_t) * count, hipMemcpyHostToDevice));
        } else {
            const std::vector<int32_t> *src[3] = {&h.cam, &h.img, &h.key};
            DevBuf *dst[3] = {&cam, &img, &key};
            for (DevBuf *b : dst)
                if (const int rc = b->grow(count, sizeof(int32_t))) return rc;
            for (int q = 0; q < 3; ++q) HIPCHK(hipMemcpy(dst[q]->p, src[q]->data(), sizeof(int32_t) * count, hipMemcpyHostToDevice));
        }
        if (const int rc = uv.grow(2 * count, f32 ? sizeof(float) : sizeof(double))) return rc;
        if (f32) {   // float measurements: the rounding happens here, on upload
            std::vector<float> f(2 * count);
            for (int64_t i = 0; i < 2 * count; ++i) f[i] = (float)uv_host[i];
            HIPCHK(hipMemcpy(uv.p, f.data(), sizeof(float) * 2 * count, hipMemcpyHostToDevice));
        } else {
            HIPCHK(hipMemcpy(uv.p, uv_host, sizeof(double) * 2 * count, hipMemcpyHostToDevice));
        }
        n = count;
        return PCS_OK;
    }

    // The table's noise weights: n checked values (the caller has validated them and waited for everything that reads the old ones), or
    // NULL = none.  They belong to the table: upload() and release() drop them.  A failed allocation or copy leaves "no weights".
    int set_weights(const double *inv_sigma) {
        w.release();
        if (!inv_sigma || n == 0) return PCS_OK;
        if (const int rc = w.grow(n, sizeof(double))) return rc;
        const hipError_t e = hipMemcpy(w.p, inv_sigma, sizeof(double) * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            w.release();
            return fail(PCS_ERR_HIP, "uploading the noise weights failed: %s", hipGetErrorString(e));
        }
        return PCS_OK;
    }
};
