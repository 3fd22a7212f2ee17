// rbf_kernels_mask_body.h -- the body of the two GOP mask kernels (k_residual_mask_gop, k_residual_mask_any_gop in rbf_kernels_mask.h).
// NOT a header: it is #included INSIDE each kernel's braces, so that both kernels are ONE function each, compiled from the same text --
// the luma kernels' instructions stay exactly what they were before the all-channel twin existed (a force-inlined shared __device__ body
// changed their scheduling).  The including kernel defines SAMPLE, PIXEL_BYTES, NT, THR0 and ANY (template parameters or constexpr
// locals) and the arguments frames, frame_stride, nframes, nsegs, thr_all, thr_tab, masks, mask_stride_u16, ones, chunks, fin.
// ANY = the all-channel bit (lane_bits_any; THR0 is then ignored): the only per-pair "threshold" it sees is the skip marker a table may
// carry for a pair in front of a keyframe (thr_tab[p] > 0: a zero row, nothing counted).
    // blockIdx.y = temporal chunk: frames [f0, f1] (f1 - f0 pairs); chunks of one run overlap by one frame, which
    // buys gridDim.y times more waves in flight for ~gridDim.y/nframes extra reads
    extern __shared__ uint32_t cnt[];                          // [nframes-1] per-workgroup ones
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t seg = (uint64_t)blockIdx.x * WG_WAVES + wave;
    uint32_t f0, f1;
    bool skipped = false;
    if (chunks.count) {
        const uint32_t c = chunks.pairs[blockIdx.y];
        f0 = chunks.first[blockIdx.y];
        f1 = f0 + (c & (MASK_CHUNK_SKIP - 1u));
        skipped = (c & MASK_CHUNK_SKIP) != 0u;
    } else {
        f0 = blockIdx.y * chunks.ppc;
        f1 = f0 + chunks.ppc < nframes - 1 ? f0 + chunks.ppc : nframes - 1;
    }
    for (uint32_t i = threadIdx.x; i + 1 < nframes; i += WG_THREADS) cnt[i] = 0;
    __syncthreads();
    if (skipped) {
        if (seg < nsegs)
            for (uint32_t f = f0; f < f1; ++f) masks[seg * 64 + lane + (uint64_t)f * mask_stride_u16] = 0;
    } else if (seg < nsegs && f0 < f1) {
        using LP = LanePixels<SAMPLE, PIXEL_BYTES>;
        const uint64_t lane_off = (seg * 1024 + (uint64_t)lane * 16) * PIXEL_BYTES;
        const uint8_t *p = frames + lane_off;
        uint16_t *out = masks + seg * 64 + lane;
        uint32_t one2;
        asm volatile("v_mov_b32 %0, 0x10001" : "=v"(one2));
        LP fa, fb, fc, fd;                                        // four frames in registers, roles rotate: TWO loads are in flight while a pair is compared
        fa.template load<NT>(p + (uint64_t)f0 * frame_stride);
        fb.template load<NT>(p + (uint64_t)(f0 + 1) * frame_stride);
        if (f0 + 2 <= f1) fc.template load<NT>(p + (uint64_t)(f0 + 2) * frame_stride);
        // pair (prev, cur) = mask f-1; `nxt2` receives frame f+2 meanwhile (frame f+1 is already on its way).  Returns a value whose
        // population count is this lane's number of set bits.
        auto step = [&](const LP &prev, const LP &cur, LP &nxt2, uint32_t f) -> uint32_t {
            if (f + 2 <= f1) nxt2.template load<NT>(p + (uint64_t)(f + 2) * frame_stride);
            const int32_t thr = thr_tab ? thr_tab[f - 1] : thr_all;
            uint32_t bits = 0, csrc = 0;
            if constexpr (ANY) {
                bits = lane_bits_any<SAMPLE, PIXEL_BYTES>(prev, cur, one2, csrc);
                if (thr > 0) bits = csrc = 0;
            } else {
                if (THR0) bits = lane_bits_thr0<SAMPLE, PIXEL_BYTES>(prev, cur, one2, csrc);      // host: no per-pair table and thr == 0
                else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const bool b = residual_bit<SAMPLE>((SAMPLE)prev.luma(k), (SAMPLE)cur.luma(k), thr);
                        bits |= (b ? 1u : 0u) << (k ^ 7);         // MSB-first within each byte
                    }
                    csrc = bits;
                }
            }
            out[(uint64_t)(f - 1) * mask_stride_u16] = (uint16_t)bits;
            return csrc;
        };
        // The wave's counts stay in ONE register until the chunk ends: lane s of `tally` holds the ones of pairs base + 2s (low half) and
        // base + 2s + 1 (high half).  Two pairs share a DPP tree (their lane counts ride as packed 16-bit halves, each total <= 1024),
        // v_readlane hands the packed totals to the scalar unit and ONE v_writelane files them.  Round 5 did a six-step tree, a compare, two exec
        // masks and the compiler's uniform-address atomic loop (~8 vector + ~15 scalar instructions and an LDS atomic) PER PAIR -- in a
        // kernel that runs underneath the issue-bound insert / query kernels of the neighbouring pipelines, where every instruction it
        // issues is one of theirs that waits.
        uint32_t tally = 0, base = f0;
        auto flush = [&]() {
            const uint32_t i = base + 2u * lane;
            if (i < f1 && (tally & 0xFFFFu)) atomicAdd(&cnt[i], tally & 0xFFFFu);     // (per-lane addresses: one ds_add_u32 for the wave)
            if (i + 1u < f1 && (tally >> 16)) atomicAdd(&cnt[i + 1u], tally >> 16);
            tally = 0;
        };
        auto file2 = [&](uint32_t c_even, uint32_t c_odd, uint32_t f) {               // counts of pairs f-1 and f
            const uint32_t tot = wave_sum_to_lane63(__popc(c_even) | (__popc(c_odd) << 16));
            const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)tot, 63);
            const uint32_t slot = (f - 1u - base) >> 1;                               // < 64 (scalar: f and base are uniform)
            uint32_t keep;
            // v_writelane takes ONE SGPR over the constant bus, so the lane select rides in M0 (reserved: saved and restored, as RowDmaC does).
            // Hazard: v_writelane must not read an SGPR that a VALU instruction (v_readlane, a ballot) wrote in the last 5 wait states -- it
            // would see the PREVIOUS value, and hipcc pads no hazards inside asm (the parity tests caught exactly that).  `t` is such an
            // SGPR: the two s_mov and the s_nop in front of the v_writelane are its distance, do not thin them out.
            asm volatile("s_mov_b32 %1, m0\n\t"
                         "s_mov_b32 m0, %3\n\t"
                         "s_nop 0\n\t"
                         "v_writelane_b32 %0, %2, m0\n\t"
                         "s_mov_b32 m0, %1"
                         : "+v"(tally), "=&s"(keep) : "s"(t), "s"(slot));
        };
        // unrolled by four so that the rotation prev <- cur <- nxt <- nxt2 costs no register moves
        for (uint32_t f = f0 + 1; f <= f1; f += 4) {
            if (f - 1u - base == 2u * WAVE) { flush(); base += 2u * WAVE; }
            const uint32_t c0 = step(fa, fb, fd, f);
            const uint32_t c1 = f + 1 <= f1 ? step(fb, fc, fa, f + 1) : 0u;
            file2(c0, c1, f);
            if (f + 2 <= f1) {
                const uint32_t c2 = step(fc, fd, fb, f + 2);
                const uint32_t c3 = f + 3 <= f1 ? step(fd, fa, fc, f + 3) : 0u;
                file2(c2, c3, f + 2);
            }
        }
        flush();
    }
    __syncthreads();
    for (uint32_t i = f0 + threadIdx.x; i < f1; i += WG_THREADS)
        if (cnt[i]) atomicAdd((unsigned long long *)&ones[i], (unsigned long long)cnt[i]);
    if (!fin.enabled) return;
    // ---- the tail of the pass (see MaskFinish).  Only wave 0 -- whose lanes issued the workgroup's count atomics -- takes a ticket.
    const uint64_t wg = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x, nwg = (uint64_t)gridDim.x * gridDim.y;
    const uint4 z = make_uint4(0, 0, 0, 0);
    const bool wide = f1 > f0 + WAVE;              // (workgroup-uniform) more than 64 pairs in this chunk: waves 1..3 issued count atomics too
    if (wide) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (wave != 0) {                               // waves 1..3: their share of the clears, and out
        for (uint64_t i = wg * WG_THREADS + threadIdx.x; i < fin.quads_a; i += nwg * WG_THREADS) fin.clear_a[i] = z;
        for (uint64_t i = wg * WG_THREADS + threadIdx.x; i < fin.quads_b; i += nwg * WG_THREADS) fin.clear_b[i] = z;
        return;
    }
    // My counts must have been performed before my ticket is.  They are agent-scope atomics (carried out at the device's coherence
    // point, not in this XCD's L2), so waiting for their acknowledgements is enough -- a __threadfence() here writes the L2 back
    // from every workgroup and made the kernel 8x slower (25 -> 190 us).
    if (!wide) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // Two-level ticket: all ~2 000 workgroups of a 1080p GOP are resident at once and finish together, and returning atomics on ONE
    // address complete one every ~6 ns -- a single counter cost the kernel 13 us.  64 first-level counters (workgroup id mod 64),
    // whose last arrivals meet on a second-level one.
    uint32_t is_last = 0;
    if (lane == 0) {
        const uint32_t idx = (uint32_t)(wg % MASK_TICKETS);
        const uint32_t mine = (uint32_t)((nwg + MASK_TICKETS - 1 - idx) / MASK_TICKETS);      // workgroups on this counter
        if (atomicAdd(fin.ticket + idx, 1u) == mine - 1u) {
            __hip_atomic_store(fin.ticket + idx, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t groups = nwg < MASK_TICKETS ? (uint32_t)nwg : (uint32_t)MASK_TICKETS;
            is_last = atomicAdd(fin.ticket + MASK_TICKETS, 1u) == groups - 1u ? 1u : 0u;
        }
    }
    is_last = __builtin_amdgcn_readfirstlane(is_last);
    for (uint64_t i = wg * WG_THREADS + threadIdx.x; i < fin.quads_a; i += nwg * WG_THREADS) fin.clear_a[i] = z;
    for (uint64_t i = wg * WG_THREADS + threadIdx.x; i < fin.quads_b; i += nwg * WG_THREADS) fin.clear_b[i] = z;
    if (!is_last) return;
    // the last workgroup: counts out (to the caller's array and the host), accumulator and ticket back to zero
    for (uint32_t i = lane; i < fin.count; i += WAVE) {
        const uint64_t v = __hip_atomic_load(&ones[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (the other workgroups added at the coherence point)
        fin.ones_out[i] = v;
        __hip_atomic_store(&ones[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fin.host_block) __hip_atomic_store(&fin.host_block[1 + i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (fin.host_block) {
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(&fin.host_block[0], fin.token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (lane == 0) __hip_atomic_store(fin.ticket + MASK_TICKETS, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
