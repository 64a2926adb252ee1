// The kernel of policy_wide.hip, as text: that file includes this one three times, inside its anonymous namespace --
//   POLICY_WIDE_KERNEL = k_policy_wide,       POLICY_WIDE_BANK = false, POLICY_WIDE_ROUTE = 0: the plain handle's kernel;
//   POLICY_WIDE_KERNEL = k_policy_wide_bank,  POLICY_WIDE_BANK = true,  POLICY_WIDE_ROUTE = 0: an actor bank's (swarm_policy_bank_create);
//   POLICY_WIDE_KERNEL = k_policy_wide_route, POLICY_WIDE_BANK = false, POLICY_WIDE_ROUTE = 1: a bank's under swarm_policy_bank_route.
// As csrc/policy_mlp_kernel.h, and for its reason: the plain kernels keep their symbols and their device code
// (tools/isa_diff.py).  BANK: blockIdx.y is the member, blockIdx.x the workgroup inside the member's R rows of the call, P.rows
// carries R; the member's streams lie one whole blob (both streams) behind the previous member's, and every bound is the
// member's end.  The noise key stays row_offset + the call's row.
// ROUTE: as csrc/policy_mlp_kernel.h says -- workgroup b serves entry b of the route's tile table (member, first slot, slot
// count), a lane's true row comes from env_order, a tile of count 0 returns before the first barrier.
template <bool IN_BF16, bool X3, bool LOGPI, int MT>
__global__ void __launch_bounds__(kThreads, (MT == 6 && !X3) ? 2 : 1)
POLICY_WIDE_KERNEL(const WideParams P, const void *__restrict__ obs_, float *__restrict__ act, float *__restrict__ log_pi, float logpi_c
#if POLICY_WIDE_ROUTE
                   , const swarm_wide::RouteView R
#endif
                   )
{
    typedef Geo<MT> G;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    bf8 *const lds = reinterpret_cast<bf8 *>(smem_raw);     // buffer b at lds + b * CH
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    constexpr bool BANK = POLICY_WIDE_BANK;
    constexpr bool ROUTE = POLICY_WIDE_ROUTE;
#if POLICY_WIDE_ROUTE
    const int4 te = R.tiles[blockIdx.x];                    // (member, first slot, slots, -)
    if (te.z <= 0) return;                                  // uniform, before the first barrier
    const int li = wave * 32 + r;                           // this lane's index in the tile
    const int slot = te.y + (li < te.z ? li : te.z - 1);
    const int senv = slot / R.rows_per_env;
    const long long rrow = (long long)R.env_order[senv] * R.rows_per_env + (slot - senv * R.rows_per_env);   // the TRUE row
    const bool rlive = li < te.z, ron = wave * 32 < te.z;
    const unsigned rmember = (unsigned)te.x;
#else
    constexpr long long rrow = 0;
    constexpr bool rlive = false, ron = false;
    constexpr unsigned rmember = 0;
#endif
    // BANK: P.rows is the MEMBER's row count R and the call's rows are [0, gridDim.y * R); this workgroup serves member blockIdx.y
    const long long first = BANK ? (long long)blockIdx.y * P.rows : 0;      // the member's first row of the call
    const long long end = BANK ? first + P.rows : P.rows;                   // one past the last row this workgroup may touch
    // (the plain kernel names P.rows at each of its three uses below, as it always has: read through this one copy its scalar
    // registers are allocated differently, and its code must not move)
    const long long row = ROUTE ? rrow : (BANK ? first : 0) + ((long long)blockIdx.x * kWaves + wave) * 32 + r;
    const bool wave_on = ROUTE ? ron : row - r < (BANK ? end : P.rows);      // idle waves still stage and take the barriers

    const int n1 = (P.in_dim + 63) >> 6;                    // layer-1 chunks: as long as the row
    const int c_out = n1 + 2 * G::KC;                       // the output chunk, the last of the stream
    constexpr int kParts = X3 ? 2 : 1;                      // X3: every chunk twice, high stream then low stream
    const int n_steps = kParts * (c_out + 1);

    bf8 pre[G::PRE];
    auto pieces_of = [&](int c) {                           // what of chunk c's slot is staged
        return c == c_out ? G::WOUT + G::TAIL : (c == 0 || c == n1 || c == n1 + G::KC) ? G::CH : G::W;
    };
    auto issue = [&](int s) {                               // step s of the stream -> registers
        if (s >= n_steps) return;
        const int c = X3 ? s >> 1 : s;
        const bf8 *src = ((X3 && (s & 1)) ? P.lo : P.hi) + (size_t)c * G::CH;
        // the member's two streams: 2 * (c_out + 1) chunk slots behind the previous member's
        if constexpr (BANK) src += (size_t)blockIdx.y * 2 * (size_t)(c_out + 1) * G::CH;
        if constexpr (ROUTE) src += (size_t)rmember * 2 * (size_t)(c_out + 1) * G::CH;
        const int n = pieces_of(c);
#pragma unroll
        for (int k = 0; k < G::PRE; ++k) { const int q = tid + k * kThreads; if (q < n) pre[k] = src[q]; }
    };
    auto commit = [&](int s) {                              // registers -> the LDS buffer of step s
        if (s >= n_steps) return;
        const int n = pieces_of(X3 ? s >> 1 : s);
        bf8 *dst = lds + (s & 1) * G::CH;
#pragma unroll
        for (int k = 0; k < G::PRE; ++k) { const int q = tid + k * kThreads; if (q < n) dst[q] = pre[k]; }
    };

    // this lane's observation row; 64 columns (4 k-steps) at a time: the raw values of the next TWO layer-1 chunks are in
    // flight, even chunks in xa and odd chunks in xo (one chunk ahead left fp32 rows waiting: 175 us instead of 87 us for bf16
    // rows at (192,180,2))
    const size_t xoff = (size_t)(ROUTE ? row : BANK ? (row < end ? row : end - 1) : (row < P.rows ? row : P.rows - 1)) * P.in_dim;
    const float *x32 = static_cast<const float *>(obs_) + xoff;
    const __bf16 *x16 = static_cast<const __bf16 *>(obs_) + xoff;
    // (the bf16 instantiations of MT = 6 on fp32 rows keep ONE chunk in flight, in xa alone: two waves per SIMD leave no
    // registers for the second -- 20 B of scratch)
    constexpr int kAhead = (MT == 6 && !X3 && !IN_BF16) ? 1 : 2;
    XRaw<IN_BF16> xa, xo;
    auto load_x = [&](XRaw<IN_BF16> &x, int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k0 = 64 * c + 16 * i + 8 * h;
            if constexpr (IN_BF16) {                        // the fragment as it lies in memory (in_dim % 8 == 0)
                bf8 z;
#pragma unroll
                for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.0f;
                x.b[i] = k0 < P.in_dim ? *reinterpret_cast<const bf8 *>(x16 + k0) : z;
            } else {                                        // in_dim is a multiple of 4
                x.f[i][0] = x.f[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 < P.in_dim) x.f[i][0] = *reinterpret_cast<const float4 *>(x32 + k0);
                if (k0 + 4 < P.in_dim) x.f[i][1] = *reinterpret_cast<const float4 *>(x32 + k0 + 4);
            }
        }
    };

    bf8 pk[G::KS];                                          // B fragments: layer 1 uses pk[0..3] for the current chunk
    bf8 pl[X3 ? G::KS : 1];                                 // X3: their low parts
    f16v acc[MT];
    auto convert_x = [&](const XRaw<IN_BF16> &x) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (IN_BF16) {
                pk[i] = x.b[i];
                if constexpr (X3) {                         // bf16 rows have no low part
#pragma unroll
                    for (int j = 0; j < 8; ++j) pl[i][j] = (__bf16)0.0f;
                }
            } else {
                const float xv[8] = {x.f[i][0].x, x.f[i][0].y, x.f[i][0].z, x.f[i][0].w, x.f[i][1].x, x.f[i][1].y, x.f[i][1].z, x.f[i][1].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const __bf16 hj = (__bf16)xv[j];
                    pk[i][j] = hj;
                    if constexpr (X3) pl[i][j] = (__bf16)(xv[j] - (float)hj);
                }
            }
        }
    };
    // the bias tail of the chunk in `wl` (at piece `off`): SET the first `tiles` accumulators to it, or ADD it (X3's low part)
    auto bias = [&](const bf8 *wl, int off, int tiles, bool add) {
        const float *bt = reinterpret_cast<const float *>(wl + off);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            if (mt < tiles) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v = *reinterpret_cast<const float4 *>(bt + 32 * mt + 8 * g + 4 * h);
                    const float bv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[mt][4 * g + e] = add ? acc[mt][4 * g + e] + bv[e] : bv[e];
                }
            }
    };
    // the MFMAs of one hidden-width chunk: 4 k-steps, B fragments b0[0..3] (and their low parts), all MT feature tiles
    // (with_lo = false: the low parts are known to be zero -- layer 1 on bf16 rows -- and their MFMAs are left out)
    auto mma = [&](const bf8 *wl, const bf8 *b0, const bf8 *l0, bool low, bool with_lo) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf8 a = wl[(mt * 4 + i) * 64 + lane];
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b0[i], acc[mt], 0, 0, 0);
                if constexpr (X3) {
                    if (!low && with_lo) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, l0[i], acc[mt], 0, 0, 0);
                }
            }
    };

    int s = 0;                                              // the step that is in LDS buffer s & 1
    issue(0);
    if (wave_on) {
        load_x(xa, 0);
        if (kAhead == 2 && 1 < n1) load_x(xo, 1);
    }
    commit(0);
    __syncthreads();

    // ---- layer 1: n1 chunks, the row's columns of the two chunks behind this one loading while its MFMAs run
    auto layer1_chunk = [&](XRaw<IN_BF16> &x, int c) {
#pragma unroll
        for (int part = 0; part < kParts; ++part) {
            const bool low = part == 1;
            issue(s + 1);
            const bf8 *wl = lds + (s & 1) * G::CH;
            if (wave_on) {
                if (!low) {
                    convert_x(x);
                    if (c + kAhead < n1) load_x(x, c + kAhead);
                    if (c == 0) bias(wl, G::W, MT, false);  // b1, fp32 (the low stream's tail of layer 1 is zero: not added)
                }
                mma(wl, pk, pl, low, !IN_BF16);
            }
            commit(s + 1);
            __syncthreads();
            ++s;
        }
    };
#pragma unroll 1
    for (int c = 0; c < n1; c += kAhead) {
        layer1_chunk(xa, c);
        if (kAhead == 2 && c + 1 < n1) layer1_chunk(xo, c + 1);
    }

    // leaky ReLU (slope 0.01, the product rounded in fp32) and the split into bf16 parts: the accumulator tile becomes the
    // next layer's B fragments, k-step = 2 * feature tile + half
    auto activate = [&]() {
#pragma unroll
        for (int kt = 0; kt < MT; ++kt)
#pragma unroll
            for (int sh = 0; sh < 2; ++sh)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = acc[kt][8 * sh + j];
                    const float r_ = fmaxf(v, 0.01f * v);
                    const __bf16 hj = (__bf16)r_;
                    pk[2 * kt + sh][j] = hj;
                    if constexpr (X3) pl[2 * kt + sh][j] = (__bf16)(r_ - (float)hj);
                }
    };

    // ---- layers 2 and 3
#pragma unroll 1
    for (int layer = 0; layer < 2; ++layer) {
        if (wave_on) activate();
#pragma unroll
        for (int kc = 0; kc < G::KC; ++kc)
#pragma unroll
            for (int part = 0; part < kParts; ++part) {
                const bool low = part == 1;
                issue(s + 1);
                const bf8 *wl = lds + (s & 1) * G::CH;
                if (wave_on) {
                    if (kc == 0) bias(wl, G::W, MT, low);   // bf(b) sets the accumulators, lo(b) is added
                    mma(wl, pk + 4 * kc, pl + (X3 ? 4 * kc : 0), low, true);
                }
                commit(s + 1);
                __syncthreads();
                ++s;
            }
    }

    // ---- output layer: one feature tile; action k is accumulator register k of the lower lane half (row = reg, h = 0)
    if (wave_on) activate();
#pragma unroll
    for (int part = 0; part < kParts; ++part) {
        const bool low = part == 1;
        issue(s + 1);
        const bf8 *wl = lds + (s & 1) * G::CH;
        if (wave_on) {
            bias(wl, G::WOUT, 1, low);
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                const bf8 a = wl[ks * 64 + lane];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pk[ks], acc[0], 0, 0, 0);
                if constexpr (X3) {
                    if (!low) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pl[ks], acc[0], 0, 0, 0);
                }
            }
        }
        if (part + 1 < kParts) {
            commit(s + 1);
            __syncthreads();
            ++s;
        }
    }
    if (wave_on && h == 0 && (ROUTE ? rlive : row < (BANK ? end : P.rows))) finish_row<LOGPI>(P, acc[0], row, act, log_pi, logpi_c);
}
