// The kernel of policy_mlp.hip, as text: that file includes this one three times, inside its anonymous namespace --
//   POLICY_MLP_KERNEL = k_policy_mlp,       POLICY_MLP_BANK = false, POLICY_MLP_ROUTE = 0: the plain handle's kernel;
//   POLICY_MLP_KERNEL = k_policy_mlp_bank,  POLICY_MLP_BANK = true,  POLICY_MLP_ROUTE = 0: an actor bank's (swarm_policy_bank_create);
//   POLICY_MLP_KERNEL = k_policy_mlp_route, POLICY_MLP_BANK = false, POLICY_MLP_ROUTE = 1: a bank's under swarm_policy_bank_route.
// Text and not a shared inlined body or one more template parameter: the plain kernels keep their symbols and compile to the
// device code they had before the bank existed, instruction for instruction (tools/isa_diff.py) -- every BANK term below
// folds away in the front end.
//
// BANK: the grid is 2-D, blockIdx.y is the MEMBER and blockIdx.x the workgroup inside the member's R rows
// [member * R, (member + 1) * R) of the call; P.rows carries R, not the call's row count.  The member's weights are the
// handle's first member's plus member * kMemberPieces pieces -- uniform per workgroup, a scalar -- and every bound (wave_on,
// the load clamp, the store predicate) is the member's END, not the call's: a tail tile of member m neither reads nor writes a
// row of member m + 1.  The noise key stays row_offset + the call's row, so the noise does not depend on the members.
//
// ROUTE (one more kernel argument, the route's tables): the grid is 1-D and workgroup b serves entry b of the tile table the
// routing kernel wrote (k_policy_route_table in policy_mlp.hip): (member, first slot, slot count).  Slots number the rows of
// the served envs in env_order; a lane's slot is first + its index in the workgroup, the tile's last slot standing in for a
// lane past the count (the clamp idiom of the other two kernels), and its TRUE row of the call is
// env_order[slot / rows_per_env] * rows_per_env + slot % rows_per_env: the observation load, the act / log_pi addresses and
// the noise key use that row, the store predicate the slot count.  A tile of count 0 (surplus of the grid's upper bound)
// returns before the first barrier, the whole workgroup.  One tile per wave only.
template <bool IN_BF16, int TPW, bool X3, bool LOGPI>
__global__ void __launch_bounds__(64 * waves_of(X3), (TPW == 1 && !X3) ? 2 : 1)
POLICY_MLP_KERNEL(const MlpParams P, const void *__restrict__ obs_, float *__restrict__ act, float *__restrict__ log_pi, float logpi_c
#if POLICY_MLP_ROUTE
                  , const swarm_wide::RouteView R
#endif
                  )
{
    constexpr int kWaves = waves_of(X3), kPre = pre_of(kWaves);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    bf8 *const buf[2] = {reinterpret_cast<bf8 *>(smem_raw), reinterpret_cast<bf8 *>(smem_raw) + kChunkFrags * 64};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    constexpr bool BANK = POLICY_MLP_BANK;
    constexpr bool ROUTE = POLICY_MLP_ROUTE;
#if POLICY_MLP_ROUTE
    static_assert(TPW == 1, "a routed tile is one wave's 32 rows");
    const int4 te = R.tiles[blockIdx.x];                                                // (member, first slot, slots, -)
    if (te.z <= 0) return;                                                              // uniform, before the first barrier
    const int li = wave * 32 + r;                                                       // this lane's index in the tile
    const int slot = te.y + (li < te.z ? li : te.z - 1);
    const int senv = slot / R.rows_per_env;
    const long long rrow = (long long)R.env_order[senv] * R.rows_per_env + (slot - senv * R.rows_per_env);   // the TRUE row
    const bool rlive = li < te.z, ron = wave * 32 < te.z;
    const int rmember = te.x;
#else
    constexpr long long rrow = 0;
    constexpr bool rlive = false, ron = false;
    constexpr int rmember = 0;
#endif
    // BANK: P.rows is the MEMBER's row count R and the call's rows are [0, gridDim.y * R); this workgroup serves member blockIdx.y
    const long long first = BANK ? (long long)blockIdx.y * P.rows : 0;                  // the member's first row of the call
    const long long end = BANK ? first + P.rows : P.rows;                               // one past the last row this workgroup may touch
    const size_t woff = ROUTE ? (size_t)rmember * kMemberPieces : BANK ? (size_t)blockIdx.y * kMemberPieces : 0;   // the member's blob, in 16-byte pieces
    const long long row0 = ROUTE ? rrow : (BANK ? first : 0) + ((long long)blockIdx.x * kWaves + wave) * (32 * TPW) + r;    // this lane's row in tile 0
    const bool wave_on = ROUTE ? ron : row0 - r < end;                                  // idle waves still stage and take the barriers

    bf8 pre[kPre];
    // chunk step cc: X3 interleaves (chunk c, high) and (chunk c, low)
    constexpr int kSteps = X3 ? 2 * kChunks : kChunks;
    auto issue = [&](int cc) {                                              // chunk step cc of the weight stream -> registers
        const int c = X3 ? cc >> 1 : cc;
        const bool low = X3 && (cc & 1);
        const bf8 *b1_ = low ? P.l1 : P.w1, *b2_ = low ? P.l2 : P.w2, *b3_ = low ? P.l3 : P.w3, *b4_ = low ? P.l4 : P.w4;
        const bf8 *w = c < 2 ? b1_ + (size_t)c * kChunkFrags * 64 : c < 4 ? b2_ + (size_t)(c - 2) * kChunkFrags * 64
                     : c < 6 ? b3_ + (size_t)(c - 4) * kChunkFrags * 64 : b4_;
        if constexpr (BANK || ROUTE) w += woff;
        const int n = (c < 6 ? kChunkFrags : kKS) * 64;
#pragma unroll
        for (int k = 0; k < kPre; ++k) { const int q = tid + k * 64 * kWaves; if (q < n) pre[k] = w[q]; }
    };
    auto commit = [&](int cc) {                                             // registers -> LDS buffer of chunk step cc
        const int c = X3 ? cc >> 1 : cc;
        const int n = (c < 6 ? kChunkFrags : kKS) * 64;
#pragma unroll
        for (int k = 0; k < kPre; ++k) { const int q = tid + k * 64 * kWaves; if (q < n) buf[cc & 1][q] = pre[k]; }
    };

    issue(0);
    // the 12 B fragments of layer 1, straight from the observation row (natural k order); later `pk` holds the packed
    // activations of the previous layer (k-step = 2 * feature tile + s)
    bf8 pk[TPW][kKS];
    bf8 pl[X3 ? TPW : 1][X3 ? kKS : 1];                                     // X3: the low parts of the activations
    f16v acc[TPW][kMT];
    if (wave_on) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const long long row = row0 + 32 * t;
            const size_t xoff = (size_t)(ROUTE ? row : (row < end ? row : end - 1)) * P.in_dim;     // (ROUTE: clamped by slot)
            const float *x = static_cast<const float *>(obs_) + xoff;
            const __bf16 *xb = static_cast<const __bf16 *>(obs_) + xoff;
#pragma unroll
            for (int ks = 0; ks < kKS; ++ks) {
                const int k0 = 16 * ks + 8 * h;
                if constexpr (IN_BF16) {                                    // the fragment as it lies in memory (in_dim % 8 == 0)
                    bf8 z;
#pragma unroll
                    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.0f;
                    pk[t][ks] = k0 < P.in_dim ? *reinterpret_cast<const bf8 *>(xb + k0) : z;
                    if constexpr (X3) pl[t][ks] = z;                        // bf16 rows have no low part
                    continue;
                }
                float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
                if (k0 < P.in_dim) lo = *reinterpret_cast<const float4 *>(x + k0);          // in_dim is a multiple of 4
                if (k0 + 4 < P.in_dim) hi = *reinterpret_cast<const float4 *>(x + k0 + 4);
                const float xv[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const __bf16 hj = (__bf16)xv[j];
                    pk[t][ks][j] = hj;
                    if constexpr (X3) pl[t][ks][j] = (__bf16)(xv[j] - (float)hj);
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float bv = ((BANK || ROUTE) ? P.b1 + 4 * woff : P.b1)[feat_of(mt, reg, h)];
#pragma unroll
                for (int t = 0; t < TPW; ++t) acc[t][mt][reg] = bv;
            }
    }
    commit(0);
    __syncthreads();

#pragma unroll
    for (int cc = 0; cc < kSteps; ++cc) {
        const int c = X3 ? cc >> 1 : cc;
        const bool low = X3 && (cc & 1);                                    // this step holds LOW weight parts
        const bool last_part = !X3 || low;                                  // the chunk's sums are complete after this step
        if (cc + 1 < kSteps) issue(cc + 1);
        const bf8 *wl = buf[cc & 1];
        if (wave_on) {
            if (c < 6) {
                const int half = c & 1;
#pragma unroll
                for (int ks = 0; ks < kKS; ++ks)
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        const bf8 a = wl[(m * kKS + ks) * 64 + lane];
#pragma unroll
                        for (int t = 0; t < TPW; ++t) {
                            acc[t][3 * half + m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pk[t][ks], acc[t][3 * half + m], 0, 0, 0);
                            if constexpr (X3) {
                                if (!low) acc[t][3 * half + m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pl[t][ks], acc[t][3 * half + m], 0, 0, 0);
                            }
                        }
                    }
                if (half == 1 && last_part) {                               // layer complete: leaky ReLU (slope 0.01, networks.py:40-42), pack
#pragma unroll
                    for (int t = 0; t < TPW; ++t) {
#pragma unroll
                        for (int kt = 0; kt < kMT; ++kt)
#pragma unroll
                            for (int s = 0; s < 2; ++s)
#pragma unroll
                                for (int j = 0; j < 8; ++j) {
                                    const float v = acc[t][kt][8 * s + j];
                                    const float r_ = fmaxf(v, 0.01f * v);
                                    const __bf16 hj = (__bf16)r_;
                                    pk[t][2 * kt + s][j] = hj;
                                    if constexpr (X3) pl[t][2 * kt + s][j] = (__bf16)(r_ - (float)hj);
                                }
#pragma unroll
                        for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
                            for (int reg = 0; reg < 16; ++reg) acc[t][mt][reg] = 0.0f;
                    }
                }
            } else {
                // output layer: one feature tile; action k is accumulator register k of the lower lane half (row = reg, h = 0)
#pragma unroll
                for (int t = 0; t < TPW; ++t) {
                    f16v o = acc[t][0];                                     // zeros (X3: the high step's sums on the low step)
#pragma unroll
                    for (int ks = 0; ks < kKS; ++ks) {
                        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[ks * 64 + lane], pk[t][ks], o, 0, 0, 0);
                        if constexpr (X3) {
                            if (!low) o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[ks * 64 + lane], pl[t][ks], o, 0, 0, 0);
                        }
                    }
                    if constexpr (X3) { if (!low) { acc[t][0] = o; continue; } }
                    const long long row = row0 + 32 * t;
                    if (h == 0 && (ROUTE ? rlive : row < end)) {
                        float *y = act + (size_t)row * P.act_dim;
                        float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (P.noise_scale > 0.0f) {
                            unsigned long long hk = pmix64(P.noise_key ^ (P.row_offset + (unsigned long long)row));
#pragma unroll
                            for (int k = 0; k < 4; k += 2) {
                                if (k < P.act_dim) {
                                    const float u1 = (float)((unsigned)(hk >> 40) + 1u) * 5.9604644775390625e-08f;      // (0, 1]
                                    const float u2 = (float)((unsigned)(hk >> 16) & 0xFFFFFFu) * 5.9604644775390625e-08f; // [0, 1)
                                    const float rad = sqrtf(-2.0f * logf(u1));
                                    float sn, cs;
                                    sincosf(6.283185307179586f * u2, &sn, &cs);
                                    z[k] = rad * cs; z[k + 1] = rad * sn;
                                    hk = pmix64(hk + 0x9E3779B97F4A7C15ull);
                                }
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < P.act_dim) {
                                float v = tanhf(o[k]);                      // networks.py:43 tanh output
                                if (P.noise_scale > 0.0f) v = fminf(fmaxf(v + P.noise_scale * z[k], -1.0f), 1.0f);
                                y[k] = v;
                            }
                        if constexpr (LOGPI) {                              // -(0.5 sum_k z_k^2) - c, the sum in k order
                            float lp = -0.0f;                               // no noise: -act_dim log(1) = -0.0
                            if (P.noise_scale > 0.0f) {
                                float s = z[0] * z[0];
#pragma unroll
                                for (int k = 1; k < 4; ++k)
                                    if (k < P.act_dim) s = s + z[k] * z[k];
                                lp = -(0.5f * s) - logpi_c;
                            }
                            log_pi[row] = lp;
                        }
                    }
                }
            }
        }
        if (cc + 1 < kSteps) {
            commit(cc + 1);                                                 // the other buffer: last read in step cc - 1, behind the barrier
            __syncthreads();
        }
    }
}
