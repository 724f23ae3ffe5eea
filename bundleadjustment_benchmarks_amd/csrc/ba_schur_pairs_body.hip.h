// The body of the persistent pair kernel (ba_kernels.hip.h, k_schur_pairs), as text: it stands in k_schur_pairs and in k_pairs_gram, whose
// first workgroups are the pair kernel's.  Text, not a function: the same statements inlined from a __device__ function compile to
// another schedule of the same arithmetic than they do in the kernel itself, and k_schur_pairs is to stay the kernel it was,
// instruction for instruction.
// The including kernel provides T and SCALED, the pair kernel's arguments by their names, and
//   BA_PAIRS_BLOCK, BA_PAIRS_GRID   the workgroup's index among the pair workgroups and their count (unsigned).
    const int lane = threadIdx.x & 63;
    // wavefront index: the workgroups with equal blockIdx % nband (one XCD, observed) own one band of the chunk list
    const int wq = ((BA_PAIRS_BLOCK % nband) * (BA_PAIRS_GRID / nband) + BA_PAIRS_BLOCK / nband) * 4 + (threadIdx.x >> 6);
    int slot = wave_ptr[wq];
    const int slot1 = wave_ptr[wq + 1];
    if (slot >= slot1) return; // (a whole wavefront leaves; the kernel has no workgroup barrier)
    // the records as a raw buffer: 32-bit byte offsets, immediate offsets in the instruction, 0 for every offset >= rec_bytes
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(rec), 0, (int)rec_bytes, 0x00020000);
    constexpr unsigned SZ = sizeof(T), RB = BA_REC * SZ, OOB = 0xfffffff0u - 64 * SZ;
    const int i = lane & 15, k = lane >> 4;
    const bool la = i < 9;
    const unsigned lane_off = 3 * i * SZ; // element (i, 0) of Z
    typedef typename ba_acc<T>::type acc_t;
    auto entry_of = [&](const int4 ci) { // this lane's entry of the chunk (lanes past the end shadow the last entry, their products are masked)
        const int n = ci.y & 0xffff;
        return ent[ci.x + (lane < n ? lane : n - 1)];
    };
    int4 ci0 = chunk_info[slot];
    int4 ci1 = chunk_info[min(slot + 1, slot1 - 1)];
    int2 en0 = entry_of(ci0);
    for (; slot < slot1; slot++) {
        const int2 en1 = entry_of(ci1);                          // next chunk's indices: arrive under this chunk's work
        const int4 ci2 = chunk_info[min(slot + 2, slot1 - 1)];   // descriptor of the chunk after next
        const int n = ci0.y & 0xffff;
        const int hi = ci0.z & 0xffff, lo = (unsigned)ci0.z >> 16, g = ci0.w;
        const bool diag = hi == lo; // (uniform) only diagonal pairs have self entries, i.e. a reduced-rhs column
        const int ia_l = en0.x, ib_l = en0.y;
        acc_t acc;
#pragma unroll
        for (int v = 0; v < 4; v++) acc[v] = 0;
        constexpr int GB = 2; // groups of four entries per batch = what one memory round trip brings in per wavefront (two batches in flight)
        struct batch_t { T a[3 * GB], d[3 * GB], b[3 * GB]; };
        auto fetch = [&](int t0, batch_t &o) { // operands of the entries 4 t0 .. 4 (t0 + GB) - 1: lane (i, k) takes entry k of each group
#pragma unroll
            for (int u = 0; u < GB; u++) {
                const int e = 4 * (t0 + u) + k;
                const bool ok = e < n;
                const int es = ok ? e : n - 1;
                const int ia = __shfl(ia_l, es, 64), ibr = __shfl(ib_l, es, 64);
                const bool self = ibr < 0; // self entry: the column observation is the row observation, ibr = ~point
                const unsigned ra = (unsigned)ia * RB, rb = (unsigned)(self ? ia : ibr) * RB;
                const unsigned oa = (ok && la) ? ra + lane_off : OOB, ob = (ok && la) ? rb + lane_off : OOB;
                const unsigned od = (ok && la) ? ra + BA_REC_DINV * SZ : OOB;
                ba_bufload3(rsrc, oa, o.a[3 * u], o.a[3 * u + 1], o.a[3 * u + 2]);
                if (SCALED) ba_bufload3(rsrc, od, o.d[3 * u], o.d[3 * u + 1], o.d[3 * u + 2]);
                ba_bufload3(rsrc, ob, o.b[3 * u], o.b[3 * u + 1], o.b[3 * u + 2]);
                if (diag && i == 9 && ok && self) { // column 9 of B: t of the point (reduced rhs)
#pragma unroll
                    for (int m = 0; m < 3; m++) o.b[3 * u + m] = tvec[(size_t)m * Ml + (~ibr)];
                }
            }
        };
        auto multiply = [&](const batch_t &o) {
#pragma unroll
            for (int q = 0; q < 3 * GB; q++) acc = ba_mfma(SCALED ? o.a[q] * o.d[q] : o.a[q], o.b[q], acc);
        };
        // two register sets, ping-pong (no copies): the next batch is in flight under the MFMAs of the current one
        const int ngroups = (n + 3) >> 2;
        batch_t b0, b1;
        fetch(0, b0);
        for (int t0 = 0;;) { // (uniform branches)
            if (t0 + GB < ngroups) fetch(t0 + GB, b1);
            multiply(b0);
            t0 += GB;
            if (t0 >= ngroups) break;
            if (t0 + GB < ngroups) fetch(t0 + GB, b0);
            multiply(b1);
            t0 += GB;
            if (t0 >= ngroups) break;
        }
        // tile element (row r, column j = i): r = ba_crow(k, v)
        if (ci0.y & BA_CHUNK_SINGLE) {
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int r = ba_crow<T>(k, v);
                if (r >= 9) continue;
                if (i < 9) {
                    T val = -acc[v];
                    if (diag) val += V[(size_t)hi * 81 + 9 * r + i];
                    S[(size_t)(9 * lo + i) * ld + 9 * hi + r] = val;
                } else if (i == 9 && diag) {
                    const T gg = gc[9 * hi + r];
                    S[(size_t)(9 * hi + r) * ld + D] = gg - acc[v];
                    S[(size_t)(9 * hi + r) * ld + D + 1] = gg;
                }
            }
        } else {
            T *o = slab + (size_t)g * BA_SLAB;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int r = ba_crow<T>(k, v);
                if (r >= 9) continue;
                if (i < 9) o[9 * r + i] = acc[v];
                else if (i == 9) o[81 + r] = acc[v];
            }
        }
        ci0 = ci1; ci1 = ci2; en0 = en1;
    }
