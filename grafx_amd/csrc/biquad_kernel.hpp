// The text of both cascade kernels; csrc/biquad.hip includes it twice:
//   BQ_STATE 0: biquad_cascade_kernel        (x, y, Bs, As, a)            every section starts from silence
//   BQ_STATE 1: biquad_cascade_state_kernel  (x, y, Bs, As, a, zi, zf)    the sections' entering states (w[-1], w[-2]) come
//               from zi and their states after sample L - 1 go to zf, both (R, Cout, K, 2) and either NULL; zi may BE zf (a
//               pair's states are read before its first tile and written in its last, by the one wave that owns the pair),
//               so neither is __restrict__.
// Included text and not a shared device function, so that the stateless kernel's machine code is what it was before the
// state entry existed (tools/kernel_asm_diff.py): inlined from a function, the same source came out of the optimiser with
// its table set-up in another order.
#ifndef BQ_STATE
#error "biquad_kernel.hpp is the kernel text of biquad.hip: define BQ_STATE to 0 or 1 before including it"
#endif

template <int RL, bool AHEAD>
#if BQ_STATE
__global__ __launch_bounds__(BQ_T) void biquad_cascade_state_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    const float* __restrict__ Bs,
                                                                    const float* __restrict__ As, BqArgs a,
                                                                    const float* zi, float* zf) {
#else
__global__ __launch_bounds__(BQ_T) void biquad_cascade_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              const float* __restrict__ Bs,
                                                              const float* __restrict__ As, BqArgs a) {
#endif
    constexpr int BQ_PW = BQ_T / RL, BQ_TILE = RL * BQ_E, STEPS = RL == 16 ? 4 : 5;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, rl = t & (RL - 1), pw = t / RL;
    SecConst* sec = reinterpret_cast<SecConst*>(smem) + pw * a.K;
    f2* rowpow = reinterpret_cast<f2*>(reinterpret_cast<SecConst*>(smem) + BQ_PW * a.K);   // (RL = 64)

    const int64_t rc0 = 2 * ((int64_t)blockIdx.x * BQ_PW + pw);
    const bool live[2] = {rc0 < a.total, rc0 + 1 < a.total};
    const float* xr[2];
    float* yr[2];
    const float *B[2], *A[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const int64_t rc = live[ch] ? rc0 + ch : (live[0] ? rc0 : 0);   // a missing partner re-reads its neighbour, stores nothing
        const int64_t r = rc / a.Cout;
        const int c = (int)(rc - r * a.Cout);
        xr[ch] = x + row_off(a.xmap, r, a.Cin == 1 ? 0 : c);
        yr[ch] = y + row_off(a.ymap, r, c);
        B[ch] = Bs + ((r * a.Cf + (a.Cf == 1 ? 0 : c)) * a.K) * 3;
        A[ch] = As + ((r * a.Cf + (a.Cf == 1 ? 0 : c)) * a.K) * 3;
    }

    // constants: lane (k, ch) of the pair's lanes takes section k + (RL / 2) j of row-channel ch
    for (int k = rl >> 1; k < a.K; k += RL / 2) {
        const int ch = rl & 1;
        const float a0 = A[ch][3 * k];
        const float a1 = A[ch][3 * k + 1] / a0, a2 = A[ch][3 * k + 2] / a0;
        M2d s = {-(double)a1, -(double)a2, 1.0, 0.0};
#pragma unroll
        for (int e = 1; e < BQ_E; e *= 2) s = mul(s, s);  // M^E
        if constexpr (RL == 64) {
            M2d pw_j = s;
            for (int j = 0; j < 16; ++j) {   // M^(E (j + 1))
                float* dst = reinterpret_cast<float*>(rowpow + (size_t)(k * 16 + j) * 4);
                dst[0 + ch] = (float)pw_j.a;
                dst[2 + ch] = (float)pw_j.b;
                dst[4 + ch] = (float)pw_j.c;
                dst[6 + ch] = (float)pw_j.d;
                pw_j = mul(pw_j, s);
            }
        }
#pragma unroll
        for (int d = 0; d < STEPS; ++d) {
            reinterpret_cast<float*>(&sec[k].step[d][0])[ch] = (float)s.a;
            reinterpret_cast<float*>(&sec[k].step[d][1])[ch] = (float)s.b;
            reinterpret_cast<float*>(&sec[k].step[d][2])[ch] = (float)s.c;
            reinterpret_cast<float*>(&sec[k].step[d][3])[ch] = (float)s.d;
            s = mul(s, s);
        }
        reinterpret_cast<float*>(&sec[k].b0)[ch] = B[ch][3 * k] / a0;
        reinterpret_cast<float*>(&sec[k].b1)[ch] = B[ch][3 * k + 1] / a0;
        reinterpret_cast<float*>(&sec[k].b2)[ch] = B[ch][3 * k + 2] / a0;
        reinterpret_cast<float*>(&sec[k].a1)[ch] = a1;
        reinterpret_cast<float*>(&sec[k].a2)[ch] = a2;
#if BQ_STATE
        float z1 = 0.0f, z2 = 0.0f;
        if (zi != nullptr && live[ch]) {
            const float* z = zi + ((rc0 + ch) * a.K + k) * 2;
            z1 = z[0];
            z2 = z[1];
        }
        reinterpret_cast<float*>(&sec[k].carry1)[ch] = z1;
        reinterpret_cast<float*>(&sec[k].carry2)[ch] = z2;
#else
        reinterpret_cast<float*>(&sec[k].carry1)[ch] = 0.0f;
        reinterpret_cast<float*>(&sec[k].carry2)[ch] = 0.0f;
#endif
    }
    __syncthreads();  // the only barrier: tables written, every pair's lanes now work alone

    using f4 = float __attribute__((ext_vector_type(4)));
    const int64_t len = live[0] ? a.L : 0;   // (a pair past the end walks nothing: the DPP rows of a wave are independent)
    // the next tile's samples are requested before the running tile's sections are worked through: a pair's tiles are a
    // sequential chain (1024 of them at L = 131072), and with few rows there are no other waves to hide a load behind
    auto load = [&](int64_t n0, f2 (&w)[BQ_E]) {
        const int64_t n = n0 + BQ_E * rl;
        const bool whole = a.vec && n + BQ_E <= a.L;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            float e[BQ_E];
            if (whole) {
#pragma unroll
                for (int j = 0; j < BQ_E / 4; ++j) {
                    const f4 q = *reinterpret_cast<const f4*>(xr[ch] + n + 4 * j);
                    e[4 * j] = q.x; e[4 * j + 1] = q.y; e[4 * j + 2] = q.z; e[4 * j + 3] = q.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) e[i] = n + i < a.L ? xr[ch][n + i] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) reinterpret_cast<float*>(&w[i])[ch] = e[i];
        }
    };
    // AHEAD (few rows): the next tile's samples are requested before the running tile's sections are worked through --
    // there are no other waves to hide a load behind.  (With rows enough to fill the chip the other waves do that, and the
    // extra registers cost more than the request ahead brings: K = 1 at 8192 stereo rows 4.2 against 5.1 ms.)
    f2 nxt[BQ_E];
    if (AHEAD && len > 0) load(0, nxt);
    for (int64_t n0 = 0; n0 < len; n0 += BQ_TILE) {
        const int64_t n = n0 + BQ_E * rl;
        const bool whole = a.vec && n + BQ_E <= a.L;
        f2 v[BQ_E], x0[BQ_E];
        if constexpr (AHEAD) {
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) v[i] = nxt[i];
            if (n0 + BQ_TILE < len) load(n0 + BQ_TILE, nxt);
        } else {
            load(n0, v);
        }
#pragma unroll
        for (int i = 0; i < BQ_E; ++i) x0[i] = v[i];

        for (int k = 0; k < a.K; ++k) {
            SecConst& q = sec[k];
            const f2 a1 = q.a1, a2 = q.a2;
            f2 in[BQ_E];
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) in[i] = a.quirk ? x0[i] : v[i];
            // 1. zero-state run of this lane's chunk
            f2 s1 = {0.0f, 0.0f}, s2 = {0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) {
                const f2 w = fma2(-a2, s2, fma2(-a1, s1, in[i]));
                s2 = s1;
                s1 = w;
            }
            // 2. inclusive scan of the chunk end states over the sixteen lanes, the tile's entering state riding along
            const f2 c1 = q.carry1, c2 = q.carry2;
            f2 i1 = s1, i2 = s2, m1, m2;
            if (rl == 0) {
                apply2(q.step[0], c1, c2, m1, m2);
                i1 += m1;
                i2 += m2;
            }
            apply2(q.step[0], dpp2<0x111>(i1), dpp2<0x111>(i2), m1, m2);   // within the 16-lane rows: the lanes a step does
            i1 += m1;                                                       // not reach read zeros
            i2 += m2;
            apply2(q.step[1], dpp2<0x112>(i1), dpp2<0x112>(i2), m1, m2);
            i1 += m1;
            i2 += m2;
            apply2(q.step[2], dpp2<0x114>(i1), dpp2<0x114>(i2), m1, m2);
            i1 += m1;
            i2 += m2;
            apply2(q.step[3], dpp2<0x118>(i1), dpp2<0x118>(i2), m1, m2);
            i1 += m1;
            i2 += m2;
            f2 nx1, nx2;
            if constexpr (RL == 64) {
                // across the four rows: lane l of a row still lacks M^(8 (l % 16 + 1)) x (the state at the end of the row
                // before).  Rows 1 and 3 take their neighbour's total (lane 15 -> next row); then lane 31 holds the true
                // state at the end of row 1, which rows 2 and 3 take (row 3 through the 128 samples of row 2).
                const f2* rp = rowpow + (size_t)(k * 16 + (rl & 15)) * 4;
                const f2 w[4] = {rp[0], rp[1], rp[2], rp[3]};
                apply2(w, dpp2<0x142, 0xa>(i1), dpp2<0x142, 0xa>(i2), m1, m2);
                i1 += m1;
                i2 += m2;
                f2 u1 = dpp2<0x143, 0xc>(i1), u2 = dpp2<0x143, 0xc>(i2);
                apply2(q.step[4], u1, u2, m1, m2);   // M^128
                if (rl >= 48) {
                    u1 = m1;
                    u2 = m2;
                }
                apply2(w, u1, u2, m1, m2);
                i1 += m1;
                i2 += m2;
                // this lane's entering state: the inclusive total of the lane below (lane 0: the carry itself)
                s1 = dpp2<0x138>(i1);
                s2 = dpp2<0x138>(i2);
                nx1 = last_lane(i1);   // the next tile's carry
                nx2 = last_lane(i2);
            } else {
                s1 = dpp2<0x111>(i1);
                s2 = dpp2<0x111>(i2);
                nx1 = dpp2<0x121>(i1);   // lane 0 <- lane 15: the next tile's carry
                nx2 = dpp2<0x121>(i2);
            }
            if (rl == 0) {
                s1 = c1;
                s2 = c2;
                q.carry1 = nx1;   // same-wave LDS accesses are ordered: read above, write here
                q.carry2 = nx2;
            }
#if BQ_STATE
            // the state after sample L - 1: NOT the carry out of the last tile when L is no multiple of the tile (that
            // is the state after the zero padding).  The lane whose chunk holds L - 1 walks to it from its true entering
            // state, the same operations as the rerun below; w[L-2] is then the value before -- the entering s1 when
            // L - 1 opens the chunk, whichever lane, tile or call (zi) it came from.
            if (zf != nullptr && n0 + BQ_TILE >= len) {
                const int last = (int)(a.L - 1 - n0);
                if (rl == last / BQ_E) {
                    f2 t1 = s1, t2 = s2, z1 = s1, z2 = s2;
#pragma unroll
                    for (int i = 0; i < BQ_E; ++i) {
                        const f2 w = fma2(-a2, t2, fma2(-a1, t1, in[i]));
                        t2 = t1;
                        t1 = w;
                        if (i == last % BQ_E) {
                            z1 = t1;
                            z2 = t2;
                        }
                    }
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        if (!live[ch]) continue;
                        float* z = zf + ((rc0 + ch) * a.K + k) * 2;
                        z[0] = ch ? z1.y : z1.x;
                        z[1] = ch ? z2.y : z2.x;
                    }
                }
            }
#endif
            // 3. rerun from the true state, numerator
            if (!a.quirk) {
                const f2 b0 = q.b0, b1 = q.b1, b2 = q.b2;
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) {
                    const f2 w = fma2(-a2, s2, fma2(-a1, s1, in[i]));
                    v[i] = fma2(b0, w, fma2(b1, s1, b2 * s2));
                    s2 = s1;
                    s1 = w;
                }
            } else {
                const f2 b0 = q.b0, cc1 = q.b1 - q.b0 * a1, cc2 = q.b2 - q.b0 * a2;  // strictly proper part
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) {
                    const f2 w = fma2(-a2, s2, fma2(-a1, s1, in[i]));
                    v[i] = fma2(b0, v[i], fma2(cc1, s1, cc2 * s2));
                    s2 = s1;
                    s1 = w;
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            if (!live[ch]) continue;
            float e[BQ_E];
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) e[i] = ch ? v[i].y : v[i].x;
            if (whole) {
#pragma unroll
                for (int j = 0; j < BQ_E / 4; ++j)
                    __builtin_nontemporal_store(f4{e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]},
                                                reinterpret_cast<f4*>(yr[ch] + n + 4 * j));
            } else {
#pragma unroll
                for (int i = 0; i < BQ_E; ++i)
                    if (n + i < a.L) yr[ch][n + i] = e[i];
            }
        }
    }
}
