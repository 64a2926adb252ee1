// Fused policy MLP for the device-resident rollout: the reference's actor
// (/root/reference/marl_llm/algorithm/utils/networks.py:6-44 -- fc1..fc4, leaky-ReLU x3, tanh out; hidden_dim = 180,
// /root/reference/marl_llm/cfg/assembly_cfg.py:185) evaluated on the env's [E*N, 192] fp32 observation rows in ONE kernel:
// bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulate), activations never leave the registers between layers.
//
// Orientation: every layer is computed transposed, H^T = W . X^T, with the 32 batch rows of a wavefront's tile on the lanes
// (MFMA column) and the output features in the 16 accumulator registers x 2 lane halves (MFMA row).  The accumulator tile
// of layer l is then directly the B operand of layer l+1 (the product sums over its ROW index): registers 8s..8s+7 of
// feature tile kt, converted pairwise to bf16, are the fragment of k-step (kt, s); inside a step the k order is permuted
// (element j of lane half h is feature 32 kt + 16 s + 8 (j >> 2) + 4 h + (j & 3)), so the weights are packed on the host
// in exactly that order -- no transposes and no cross-lane movement of activations in the whole network (LDS only holds
// the weights).
// Fragment maps (cdna_hip_programming.md section 3): A[row = l & 31][k = 8 (l >> 5) + j], B[k = 8 (l >> 5) + j][col = l & 31],
// C/D col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
//
// Numerics: weights and layer inputs are rounded to bf16 (round-to-nearest-even), sums are fp32, layer 1's bias is fp32 and
// the biases of layers 2-4 are bf16 (the constant-one column); include/swarm_policy.h states the contract exactly and
// tests/test_gpu_policy_contract.py holds the kernel to a float64 model of it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "swarm_policy.h"
#include "swarm_internal.h"
#include "policy_wide.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
typedef __attribute__((ext_vector_type(16))) float f16v;

constexpr int kKP = 192;          // padded input / hidden width: 12 k-steps of 16, 6 feature tiles of 32
constexpr int kKS = kKP / 16;     // k-steps per layer
constexpr int kMT = kKP / 32;     // feature tiles per hidden layer
// wavefronts (32-row tiles) per workgroup = rows that share one pass of the weight stream.  bf16: four (eight: +3 %);
// bf16x3 -- twice the weight stream -- eight (155 / 179 us on 262144 bf16 / fp32 rows instead of 200 / 221 with four)
constexpr int waves_of(bool x3) { return x3 ? 8 : 4; }

struct MlpParams {
    const bf8 *w1, *w2, *w3, *w4;          // packed fragments: [feature tile][k-step][lane] x 8 bf16
    const bf8 *l1, *l2, *l3, *l4;          // the same layout, LOW parts w - bf16(w) (precision mode bf16x3 only)
    const float *b1, *b2, *b3, *b4;        // padded biases (kKP, kKP, kKP, 32)
    int in_dim, act_dim;
    long long rows;
    // exploration noise of the rollout (agents.py:93-96: action += scale * N(0, 1); clamp to [-1, 1]), fused into the epilogue:
    // counter-based generator keyed by (seed, step, row_offset + row), two normals per hash (Box-Muller)
    float noise_scale;
    unsigned long long noise_key;      // mix64(seed, step), host-side
    unsigned long long row_offset;     // global index of row 0 of this call (a rank's shard of the batch)
};

using swarm_internal::DeviceGuard;
using swarm_internal::pmix64;
using swarm_internal::swarm_noise_key;

__device__ __forceinline__ int feat_of(int mt, int reg, int h) { return 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// A workgroup = kWaves wavefronts, one 32-row tile each.  The packed weights stream through LDS in CHUNKS of three feature
// tiles (36 fragments = 36 KB; the output layer's 12 fragments are the last chunk), two LDS buffers: while the waves run
// the MFMAs of chunk c out of one buffer, every thread already holds chunk c+1 in registers (9 x 16 B, global loads issued
// before the MFMA loop) and writes it to the other buffer afterwards -- one barrier per chunk, the L2 latency of the weight
// stream hidden behind the matrix cores.  (Measured at 262144 rows: weights straight from L2 per wave 248 us; whole layers
// staged with the waves waiting 136 us, of which 47 us staging and 50 us observation loads.)
// Biases: layer 1's initialise the accumulators; for the later layers the (padded) hidden feature kOne is held at 1.0 --
// bias 1 / zero weights in layer 1, a 1.0 on the diagonal afterwards -- and the biases sit in that column of the packed
// weights (bf16, as under torch.autocast), so no bias loads in the chain.
constexpr int kChunkFrags = 3 * kKS;                                        // 36 fragments
constexpr int kChunks = 7;                                                  // 2 per hidden layer + the output layer
constexpr int pre_of(int waves) { return (kChunkFrags * 64 + 64 * waves - 1) / (64 * waves); }   // 16-byte pieces per thread and chunk
constexpr int kSmemBytes = 2 * kChunkFrags * 64 * 16;                       // 72 KB

// TPW = row tiles (32 rows each) per wave.  With one tile every MFMA needs its own 1 KB weight-fragment read from LDS (four
// SIMDs at full MFMA rate would ask for exactly the LDS bandwidth, 128 B/clk); with two tiles each read feeds two MFMAs at
// the price of ~390 VGPRs, i.e. one wave per SIMD -- measured slower, so TPW = 1 is what runs (see swarm_policy_forward).
// X3 ("bf16x3"): every operand is split into a bf16 high part and a bf16 low part (x = hi + lo to 16 significant bits) and a
// product is three MFMAs, w_hi x_hi + w_hi x_lo + w_lo x_hi, accumulated in fp32 -- the rollout then follows the reference's
// fp32 actor to ~1e-4 instead of bf16's 4e-2.  The weight stream alternates high and low chunks (same chunk size, same two
// LDS buffers: twice as many chunk steps); a high chunk meets both activation parts, a low chunk the high part only.
// LOGPI: also write log_pi[row], the log-density of the row's Gaussian exploration noise (include/swarm_policy.h).  A template
// parameter rather than a run-time test, so that the instantiations without it compile exactly as before (218 VGPRs).
//
// The kernel itself is csrc/policy_mlp_kernel.h, compiled three times: k_policy_mlp for a plain handle, k_policy_mlp_bank for
// an actor bank (BANK: blockIdx.y is the member; swarm_policy_bank_create), k_policy_mlp_route for a bank under a route (ROUTE:
// workgroup b serves entry b of the route's tile table; swarm_policy_bank_route) -- that file says why it is text and not a
// template.
constexpr size_t kMemberPieces = ((3 * kMT * kKS + kKS) * 64 * 2 * 16 + (3 * kKP + 32) * 4) / 16;   // a member's blob: high, low, biases
#define POLICY_MLP_KERNEL k_policy_mlp
#define POLICY_MLP_BANK false
#define POLICY_MLP_ROUTE 0
#include "policy_mlp_kernel.h"
#undef POLICY_MLP_KERNEL
#undef POLICY_MLP_BANK
#define POLICY_MLP_KERNEL k_policy_mlp_bank
#define POLICY_MLP_BANK true
#include "policy_mlp_kernel.h"
#undef POLICY_MLP_KERNEL
#undef POLICY_MLP_BANK
#undef POLICY_MLP_ROUTE
#define POLICY_MLP_KERNEL k_policy_mlp_route
#define POLICY_MLP_BANK false
#define POLICY_MLP_ROUTE 1
#include "policy_mlp_kernel.h"
#undef POLICY_MLP_KERNEL
#undef POLICY_MLP_BANK
#undef POLICY_MLP_ROUTE

// swarm_policy_load_device's packer: the whole blob of a handle re-written from fp32 DEVICE weights (torch.nn.Linear layout),
// in the layout swarm_policy_create packs on the host -- which stays the independent witness: tests/test_gpu_policy_load.py
// compares the two blobs byte for byte.  One thread per 16-byte piece (fragment x lane: 8 bf16 of one output feature), writing
// the piece's high and low parts; the threads behind them write the fp32 bias block.  The padded [out][in] matrices the host
// code materialises for layers 2-4 are evaluated per element: the weight where both indices are live, the bias in column
// `hidden`, the 1.0 that carries the constant-one feature at (hidden, hidden) of layers 2-3, zero elsewhere.
struct PackParams {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;      // fc1..fc4, device
    uint4 *hi, *lo;                    // the blob's high and low parts, kPackPieces 16-byte pieces each
    float *bias;                       // the blob's fp32 block, kPackBias floats
    int in_dim, hidden, act_dim;
};
constexpr int kPackPieces = (3 * kMT * kKS + kKS) * 64;                     // 228 fragments x 64 lanes
constexpr int kPackBias = 3 * kKP + 32;
constexpr int kPackThreads = 256;

// round-to-nearest-even on the bit pattern, as the host packer's bf16_rne (integer: no conversion's denormal mode to trust)
__device__ __forceinline__ unsigned pack_bf16(float f)
{
    unsigned u = __float_as_uint(f);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (u >> 16) | 0x40u;     // NaN (outside the contract)
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_policy_pack(const PackParams P)
{
    const int q = blockIdx.x * THREADS + threadIdx.x;
    if (q >= kPackPieces) {
        const int t = q - kPackPieces;                                      // bias block: b1, the constant one, zeros
        if (t < kPackBias) P.bias[t] = t < P.hidden ? P.b1[t] : (t == P.hidden ? 1.0f : 0.0f);
        return;
    }
    const int f = q >> 6, lane = q & 63, h = lane >> 5;
    const int layer = f < 3 * kMT * kKS ? f / (kMT * kKS) : 3;              // 0..3 = fc1..fc4
    const int fl = f - layer * (kMT * kKS), mt = fl / kKS, ks = fl - mt * kKS;
    const int o = 32 * mt + (lane & 31), one = P.hidden;
    const float *__restrict__ w = layer == 0 ? P.w1 : layer == 1 ? P.w2 : layer == 2 ? P.w3 : P.w4;
    const float *__restrict__ b = layer == 1 ? P.b2 : layer == 2 ? P.b3 : P.b4;       // layer 1's bias stays fp32, in the bias block
    const int n_out = layer == 3 ? P.act_dim : P.hidden;                    // live output features of this layer
    unsigned hv[8], lv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = 0.0f;
        if (layer == 0) {                                                   // natural k order, fp32 bias kept apart
            const int k = 16 * ks + 8 * h + j;
            if (o < n_out && k < P.in_dim) v = w[(size_t)o * P.in_dim + k];
        } else {                                                            // the accumulator tile's k order
            const int k = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
            if (o < n_out) { if (k < one) v = w[(size_t)o * one + k]; else if (k == one) v = b[o]; }
            else if (layer != 3 && o == one && k == one) v = 1.0f;
        }
        hv[j] = pack_bf16(v);
        lv[j] = pack_bf16(v - __uint_as_float(hv[j] << 16));                // the IEEE fp32 difference, denormals kept
    }
    P.hi[q] = make_uint4(hv[0] | hv[1] << 16, hv[2] | hv[3] << 16, hv[4] | hv[5] << 16, hv[6] | hv[7] << 16);
    P.lo[q] = make_uint4(lv[0] | lv[1] << 16, lv[2] | lv[3] << 16, lv[4] | lv[5] << 16, lv[6] | lv[7] << 16);
}

thread_local std::string g_policy_error;

// The kernels a forward call chooses from, per kernel text: [x3][in_bf16][log_pi]; the two-tile measurement instantiations
// (SWARM_POLICY_TPW=2: plain handles at bf16 only) are a table of their own, [in_bf16][log_pi].
using MlpKernel = void (*)(MlpParams, const void *, float *, float *, float);
using MlpRouteKernel = void (*)(MlpParams, const void *, float *, float *, float, swarm_wide::RouteView);
#define MLP_KERNELS(K, TPW, X3) {{K<false, TPW, X3, false>, K<false, TPW, X3, true>}, {K<true, TPW, X3, false>, K<true, TPW, X3, true>}}
const MlpKernel kPlain[2][2][2] = {MLP_KERNELS(k_policy_mlp, 1, false), MLP_KERNELS(k_policy_mlp, 1, true)};
const MlpKernel kPlainTpw2[2][2] = MLP_KERNELS(k_policy_mlp, 2, false);
const MlpKernel kBank[2][2][2] = {MLP_KERNELS(k_policy_mlp_bank, 1, false), MLP_KERNELS(k_policy_mlp_bank, 1, true)};
const MlpRouteKernel kRoute[2][2][2] = {MLP_KERNELS(k_policy_mlp_route, 1, false), MLP_KERNELS(k_policy_mlp_route, 1, true)};
#undef MLP_KERNELS

// ---- swarm_policy_bank_route's kernel: the route's tables from member_of_env, for both geometries.
// One workgroup.  Wave 0 walks the envs twice in blocks of 64, one env per lane: a lane's key is its env's member, `members`
// for an env nobody serves, members + 1 for a lane past n_env; the lanes that hold its key (nine ballots, one per key bit)
// give its rank among them and their number.  Pass 1 adds that number to the key's count in LDS (the lowest lane of each key:
// distinct keys, distinct addresses -- no atomics); one thread then turns the counts into first positions (exclusive prefix
// by member) and, per tile size, into first tiles; pass 2 places env e at first position of its key + envs of that key seen
// in earlier blocks + rank: by member, ascending env inside a member -- numpy's stable argsort, a pure function of the table.
// Meanwhile the other waves (and wave 0 behind them) write the tile tables: entry b = (member, first slot, slot count, 0) by a
// binary search of b in the members' first tiles; the entries behind the last tile carry count 0.
struct RouteTableParams {
    const int32_t *member_of_env;      // [n_env], device
    int32_t *counts;                   // [SWARM_POLICY_BANK_MAX + 1]: envs per member, the unserved count in the last word
    int32_t *env_order;                // [served envs]
    int4 *tiles[2];                    // one table per tile size
    int t_rows[2], n_tiles[2];         // rows per tile (0: no such table) and entries = rows / T + min(members, n_env)
    int n_env, rows_per_env, members;
};

template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_policy_route_table(const RouteTableParams P)
{
    constexpr int kM = SWARM_POLICY_BANK_MAX;
    __shared__ int run[kM + 2];                    // per key: the count (pass 1), then the next free position (pass 2)
    __shared__ int cnt[kM], first[kM], tbase[2][kM + 1];
    const int tid = threadIdx.x, lane = tid & 63, M = P.members;
    for (int i = tid; i < kM + 2; i += THREADS) run[i] = 0;
    __syncthreads();
    // one block of 64 envs: this lane's env and key, its rank among the lanes of its key, their number and their lowest lane
    auto block = [&](int e0, int &e, int &key, int &rank, int &n, int &lead) {
        e = e0 + lane;
        key = M + 1;
        if (e < P.n_env) { const int m = P.member_of_env[e]; key = (m >= 0 && m < M) ? m : M; }
        unsigned long long peers = ~0ull;
#pragma unroll
        for (int b = 0; b < 9; ++b) {                                       // keys < 2^9
            const bool bit = (key >> b) & 1;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        rank = __popcll(peers & ((1ull << lane) - 1ull));
        n = __popcll(peers);
        lead = __ffsll((long long)peers) - 1;
    };
    int e, key, rank, n, lead;
    if (tid < 64) {
        for (int e0 = 0; e0 < P.n_env; e0 += 64) {
            block(e0, e, key, rank, n, lead);
            if (lane == lead) run[key] += n;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int pos = 0, tb[2] = {0, 0};
        for (int m = 0; m < M; ++m) {
            const int c = run[m], rows_m = c * P.rows_per_env;             // <= n_env * rows_per_env < 2^31
            cnt[m] = c; first[m] = pos;
            pos += c;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                tbase[g][m] = tb[g];
                if (P.t_rows[g]) tb[g] += rows_m / P.t_rows[g] + (rows_m % P.t_rows[g] != 0);
            }
        }
        tbase[0][M] = tb[0]; tbase[1][M] = tb[1];
        P.counts[kM] = run[M];                                              // the unserved envs
    }
    __syncthreads();
    for (int m = tid; m < M; m += THREADS) { P.counts[m] = cnt[m]; run[m] = first[m]; }
    __syncthreads();
    if (tid < 64) {
        for (int e0 = 0; e0 < P.n_env; e0 += 64) {
            block(e0, e, key, rank, n, lead);
            int base = 0;
            if (lane == lead) { base = run[key]; run[key] = base + n; }     // the leader alone touches LDS
            base = __shfl(base, lead);
            // (the bound holds whenever the table is the one pass 1 counted; it keeps a table rewritten under the kernel inside)
            if (key < M && base + rank < P.n_env) P.env_order[base + rank] = e;
        }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!P.t_rows[g]) continue;
        const int T = P.t_rows[g], total = tbase[g][M];
        for (int b = tid; b < P.n_tiles[g]; b += THREADS) {
            int4 te = make_int4(0, 0, 0, 0);
            if (b < total) {
                int lo = 0, hi = M - 1;                                     // the last member whose first tile is <= b: it owns b
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tbase[g][mid] <= b) lo = mid; else hi = mid - 1; }
                const int j = b - tbase[g][lo], rows_m = cnt[lo] * P.rows_per_env;
                te = make_int4(lo, first[lo] * P.rows_per_env + j * T, min(T, rows_m - j * T), 0);
            }
            P.tiles[g][b] = te;
        }
    }
}

constexpr int kRouteThreads = 256;

// The blob of one actor as swarm_policy_create uploads it (and a bank holds once per member): [w1 | w2 | w3 | w4] fragments
// (8 bf16 per lane), their low parts in the same layout, then [b1 | b2 | b3 | b4] fp32.
constexpr size_t kFrag = 64 * 8;                                              // bf16 elements per fragment
constexpr size_t kHidElems = (size_t)kMT * kKS * kFrag, kOutElems = (size_t)kKS * kFrag;
constexpr size_t kWElems = 3 * kHidElems + kOutElems;
constexpr size_t kBlobBytes = 2 * kWElems * 2 + (3 * kKP + 32) * 4;           // high parts, low parts, biases
static_assert(kBlobBytes == kMemberPieces * 16 && kWElems / 8 == (size_t)kPackPieces && kPackBias == 3 * kKP + 32, "a member's blob is whole pieces");

uint16_t bf16_rne(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

std::vector<unsigned char> pack_host(const float *const w[8], int in_dim, int hidden, int act_dim)
{
    const float *w1 = w[0], *b1 = w[1], *w2 = w[2], *b2 = w[3], *w3 = w[4], *b3 = w[5], *w4 = w[6], *b4 = w[7];
    const size_t n_hid = kHidElems, w_elems = kWElems;
    std::vector<unsigned char> blob(kBlobBytes, 0);
    uint16_t *wp = reinterpret_cast<uint16_t *>(blob.data());
    uint16_t *lp = wp + w_elems;                                              // low parts: bf16(w - bf16(w)), same layout
    float *bp = reinterpret_cast<float *>(blob.data() + 2 * w_elems * 2);
    auto bf16_val = [](uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; std::memcpy(&f, &u, 4); return f; };
    // k index of fragment element j of lane half h in k-step ks: natural for layer 1 (B comes from memory), permuted for
    // the layers whose B operand is the previous accumulator tile
    auto k_nat = [](int ks, int h, int j) { return 16 * ks + 8 * h + j; };
    auto k_acc = [](int ks, int h, int j) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3); };
    auto pack = [&](uint16_t *dst, const float *w, int n_out_feat, int n_in, int tiles, bool natural) {
        uint16_t *dlo = lp + (dst - wp);
        for (int mt = 0; mt < tiles; ++mt)
            for (int ks = 0; ks < kKS; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int o = 32 * mt + (lane & 31), h = lane >> 5;
                        const int k = natural ? k_nat(ks, h, j) : k_acc(ks, h, j);
                        const float v = (o < n_out_feat && k < n_in) ? w[(size_t)o * n_in + k] : 0.0f;   // torch Linear: [out][in]
                        const size_t q = ((size_t)(mt * kKS + ks) * 64 + lane) * 8 + j;
                        dst[q] = bf16_rne(v);
                        dlo[q] = bf16_rne(v - bf16_val(dst[q]));
                    }
    };
    // The padded hidden feature `one` carries the constant 1.0 through the chain: layer 1 produces it (zero weights, bias 1),
    // the later layers copy it (1.0 on the diagonal) and read their biases from its weight column.
    const int one = hidden;
    auto with_bias = [&](const float *w, const float *b, int n_out_feat, bool keep_one) {
        std::vector<float> a((size_t)kKP * kKP, 0.0f);                      // [out][in], in padded to kKP
        for (int o = 0; o < n_out_feat; ++o) {
            for (int k = 0; k < hidden; ++k) a[(size_t)o * kKP + k] = w[(size_t)o * hidden + k];
            a[(size_t)o * kKP + one] = b[o];
        }
        if (keep_one) a[(size_t)one * kKP + one] = 1.0f;
        return a;
    };
    pack(wp, w1, hidden, in_dim, kMT, true);
    { const std::vector<float> a = with_bias(w2, b2, hidden, true); pack(wp + n_hid, a.data(), kKP, kKP, kMT, false); }
    { const std::vector<float> a = with_bias(w3, b3, hidden, true); pack(wp + 2 * n_hid, a.data(), kKP, kKP, kMT, false); }
    { const std::vector<float> a = with_bias(w4, b4, act_dim, false); pack(wp + 3 * n_hid, a.data(), kKP, kKP, 1, false); }
    for (int k = 0; k < hidden; ++k) bp[k] = b1[k];
    bp[one] = 1.0f;
    return blob;
}

bool narrow_shape_ok(int in_dim, int hidden, int act_dim)
{
    return !(in_dim < 4 || in_dim > kKP || (in_dim & 3) || hidden < 1 || hidden >= kKP || act_dim < 1 || act_dim > 4);
}

// the kernel's pointers into a handle's (first member's) blob at `base`
void point_params(MlpParams &p, const unsigned char *base, int in_dim, int act_dim)
{
    const bf8 *wd = reinterpret_cast<const bf8 *>(base);
    const float *bd = reinterpret_cast<const float *>(base + 2 * kWElems * 2);
    p.w1 = wd; p.w2 = wd + kHidElems / 8; p.w3 = wd + 2 * kHidElems / 8; p.w4 = wd + 3 * kHidElems / 8;
    const bf8 *ld = wd + kWElems / 8;
    p.l1 = ld; p.l2 = ld + kHidElems / 8; p.l3 = ld + 2 * kHidElems / 8; p.l4 = ld + 3 * kHidElems / 8;
    p.b1 = bd; p.b2 = bd + kKP; p.b3 = bd + 2 * kKP; p.b4 = bd + 3 * kKP;
    p.in_dim = in_dim; p.act_dim = act_dim; p.rows = 0; p.noise_scale = 0.0f; p.noise_key = 0; p.row_offset = 0;
}

}  // namespace

struct SWARM_HIDDEN swarm_policy {     // hidden: its implicit destructor must not become an exported weak symbol
    int device, in_dim, hidden, act_dim;
    int precision = 0;             // 0 = bf16 (default), 1 = bf16x3
    // the packed weights and biases of either geometry: `members` blobs of blob_bytes each, one behind the other
    swarm_internal::DevBuf<unsigned char> d_blob;
    size_t blob_bytes = 0;
    int members = 1;
    bool wide = false;             // the handle runs csrc/policy_wide.hip on the stream layout `wl`; p stays empty
    swarm_wide::Layout wl{};
    MlpParams p{};                 // the narrow kernel's pointers into the first member's blob
    bool smem_set = false;
    bool bank = false;             // swarm_policy_bank_create: the handle runs the BANK kernels, also with one member
    // swarm_policy_bank_route: the route in force (n_env == 0: none) and its tables, one allocation of int32 words cut for
    // cap_rows rows: [counts: SWARM_POLICY_BANK_MAX + 1][env_order: cap_rows][tile table per tile size: 4 words an entry].
    // The narrow geometry keeps two tile tables (128 rows a workgroup at bf16, 256 at bf16x3: swarm_policy_set_precision may
    // change under a route), the wide one (128 at both precisions).
    struct Route {
        int n_env = 0, rows_per_env = 0;
        long long cap_rows = 0;
        swarm_internal::DevBuf<int32_t> d_tab;
        size_t off_order = 0, off_tiles[2] = {0, 0};
        int t_rows[2] = {0, 0};
        unsigned grid(int g, int members) const
        {
            const long long rows = (long long)n_env * rows_per_env;
            return (unsigned)(rows / t_rows[g] + (members < n_env ? members : n_env));
        }
    } route;
    unsigned char *member_blob(int member) const { return d_blob.get() + (size_t)member * blob_bytes; }
};

int swarm_internal_policy_info(const swarm_policy_t *p, swarm_policy_info *out)
{
    if (!p || !out) return SWARM_POLICY_ERR_INVALID;
    out->device = p->device; out->in_dim = p->in_dim; out->act_dim = p->act_dim; out->members = p->members;
    out->route_n_env = p->route.n_env; out->route_rows_per_env = p->route.rows_per_env;
    return SWARM_POLICY_OK;
}

namespace {

// A fresh allocation filled from host memory on a stream of its own, waited for here: no null-stream work
// (tests/test_stream_sources.py), complete on return.
hipError_t upload(swarm_internal::DevBuf<unsigned char> &dst, const std::vector<unsigned char> &src)
{
    hipStream_t up = nullptr;
    hipError_t e = dst.alloc(src.size());
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(dst.get(), src.data(), src.size(), hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);
    if (up) (void)hipStreamDestroy(up);
    return e;
}

// What the three creation entry points share.  w[8 m + i]: fc1.weight, fc1.bias, ..., fc4.bias of member m (fp32, HOST); the
// entry point `who` has checked `out`, the table and its own arguments.  Here: the shape, the device, then every member's blob
// from the same host packer, one behind the other.
int create_handle(const char *who, const float *const *w, int members, int in_dim, int hidden, int act_dim, bool wide, bool bank,
                  int device, swarm_policy_t **out)
{
    const std::string pre = std::string(who) + ": ";
    if (wide ? !swarm_wide::shape_ok(in_dim, hidden, act_dim) : !narrow_shape_ok(in_dim, hidden, act_dim)) {
        g_policy_error = pre + "supported shapes " + (!bank ? "" : wide ? "of the wide geometry " : "of the narrow geometry ") + "are " +
                         (wide ? "in_dim <= 384 (multiple of 4), hidden <= 256, act_dim <= 4" : "in_dim <= 192 (multiple of 4), hidden <= 191, act_dim <= 4");
        return SWARM_POLICY_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_policy_error = pre + "no HIP device (there is no CPU path)"; return SWARM_POLICY_ERR_HIP; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    const DeviceGuard guard(device < ndev ? device : -1);       // -1 is no device: !ok
    if (!guard.ok) { g_policy_error = pre + "bad device"; return SWARM_POLICY_ERR_HIP; }
    swarm_policy *p = new (std::nothrow) swarm_policy;
    if (!p) { g_policy_error = pre + "out of memory"; return SWARM_POLICY_ERR_INVALID; }
    p->device = device; p->in_dim = in_dim; p->hidden = hidden; p->act_dim = act_dim;
    p->wide = wide; p->bank = bank; p->members = members;
    if (wide) p->wl = swarm_wide::layout_of(in_dim, hidden, act_dim);
    std::vector<unsigned char> blob;
    for (int m = 0; m < members; ++m) {
        const std::vector<unsigned char> one = wide ? swarm_wide::pack_host(p->wl, w + 8 * m) : pack_host(w + 8 * m, in_dim, hidden, act_dim);
        if (m == 0) { p->blob_bytes = one.size(); blob.reserve((size_t)members * one.size()); }
        blob.insert(blob.end(), one.begin(), one.end());
    }
    if (upload(p->d_blob, blob) != hipSuccess) {
        delete p;
        g_policy_error = pre + "device allocation / upload failed";
        return SWARM_POLICY_ERR_HIP;
    }
    if (!wide) point_params(p->p, p->d_blob.get(), in_dim, act_dim);
    *out = p;
    return SWARM_POLICY_OK;
}

// The packing launch of swarm_policy_load_device / swarm_policy_bank_load_device: member `member`'s slice of the blob.
int load_member(const char *who, swarm_policy_t *p, int member, const float *const w[8], void *stream)
{
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = std::string(who) + ": hipSetDevice failed"; return SWARM_POLICY_ERR_HIP; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p->wide) swarm_wide::load_device(p->wl, p->member_blob(member), w, st);
    else {
        static_assert(kPackPieces % 64 == 0 && sizeof(bf8) == sizeof(uint4), "one 16-byte piece per fragment lane");
        PackParams q;
        q.w1 = w[0]; q.b1 = w[1]; q.w2 = w[2]; q.b2 = w[3]; q.w3 = w[4]; q.b3 = w[5]; q.w4 = w[6]; q.b4 = w[7];
        q.hi = reinterpret_cast<uint4 *>(p->member_blob(member));
        q.lo = q.hi + kPackPieces;
        q.bias = reinterpret_cast<float *>(q.lo + kPackPieces);
        q.in_dim = p->in_dim; q.hidden = p->hidden; q.act_dim = p->act_dim;
        const unsigned grid = (kPackPieces + kPackBias + kPackThreads - 1) / kPackThreads;
        hipLaunchKernelGGL(k_policy_pack<kPackThreads>, dim3(grid), dim3(kPackThreads), 0, st, q);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_policy_error = std::string(who) + ": " + hipGetErrorString(e); return SWARM_POLICY_ERR_HIP; }
    return SWARM_POLICY_OK;
}

// swarm_policy_read_packed / swarm_policy_bank_read_packed: member `member`'s slice, on the stream, waited for.
int64_t read_member(const char *who, swarm_policy_t *p, int member, void *host_dst, int64_t capacity, void *stream)
{
    const int64_t bytes = (int64_t)p->blob_bytes;
    if (!host_dst || capacity < bytes) return bytes;
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = std::string(who) + ": hipSetDevice failed"; return -SWARM_POLICY_ERR_HIP; }
    hipStream_t st = static_cast<hipStream_t>(stream);          // the copy on the stream, behind the loads enqueued there; then the wait
    hipError_t e = hipMemcpyAsync(host_dst, p->member_blob(member), p->blob_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { g_policy_error = std::string(who) + ": " + hipGetErrorString(e); return -SWARM_POLICY_ERR_HIP; }
    return bytes;
}

}  // namespace

extern "C" {

const char *swarm_policy_last_error(void) { return g_policy_error.c_str(); }

int swarm_policy_create(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                        const float *w4, const float *b4, int in_dim, int hidden, int act_dim, int device, swarm_policy_t **out)
{
    if (!out) return SWARM_POLICY_ERR_INVALID;
    *out = nullptr;
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) { g_policy_error = "swarm_policy_create: null weight pointer"; return SWARM_POLICY_ERR_INVALID; }
    const float *const w[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    return create_handle("swarm_policy_create", w, 1, in_dim, hidden, act_dim, false, false, device, out);
}

int swarm_policy_create_wide(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                             const float *w4, const float *b4, int in_dim, int hidden, int act_dim, int device, swarm_policy_t **out)
{
    if (!out) return SWARM_POLICY_ERR_INVALID;
    *out = nullptr;
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) { g_policy_error = "swarm_policy_create_wide: null weight pointer"; return SWARM_POLICY_ERR_INVALID; }
    const float *const w[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    return create_handle("swarm_policy_create_wide", w, 1, in_dim, hidden, act_dim, true, false, device, out);
}

int swarm_policy_bank_create(const float *const *w, int members, int in_dim, int hidden, int act_dim, int wide, int device,
                             swarm_policy_t **out)
{
    if (!out) { g_policy_error = "swarm_policy_bank_create: null out"; return SWARM_POLICY_ERR_INVALID; }
    *out = nullptr;
    if (members < 1 || members > SWARM_POLICY_BANK_MAX) {
        g_policy_error = "swarm_policy_bank_create: members " + std::to_string(members) + " outside [1, " + std::to_string(SWARM_POLICY_BANK_MAX) + "]";
        return SWARM_POLICY_ERR_INVALID;
    }
    if (wide != 0 && wide != 1) { g_policy_error = "swarm_policy_bank_create: wide must be 0 (narrow geometry) or 1 (wide geometry)"; return SWARM_POLICY_ERR_INVALID; }
    if (!w) { g_policy_error = "swarm_policy_bank_create: null weight table"; return SWARM_POLICY_ERR_INVALID; }
    for (int i = 0; i < 8 * members; ++i)
        if (!w[i]) {
            g_policy_error = "swarm_policy_bank_create: null weight pointer (member " + std::to_string(i / 8) + ", array " + std::to_string(i % 8) + ")";
            return SWARM_POLICY_ERR_INVALID;
        }
    return create_handle("swarm_policy_bank_create", w, members, in_dim, hidden, act_dim, wide != 0, true, device, out);
}

int swarm_policy_bank_members(const swarm_policy_t *p) { return p ? p->members : 0; }

void swarm_policy_destroy(swarm_policy_t *p)
{
    if (!p) return;
    const DeviceGuard guard(p->device);
    delete p;
}

// log_pi != NULL: the LOGPI instantiation writes log_pi[rows] (the caller has checked the pointer).
static int policy_forward(swarm_policy_t *p, const void *obs, bool in_bf16, int64_t rows, float *act, void *stream,
                          float noise_scale = 0.0f, uint64_t seed = 0, uint64_t step = 0, uint64_t row_offset = 0,
                          float *log_pi = nullptr)
{
    if (!p || !obs || !act || rows < 0) { g_policy_error = "swarm_policy_forward: bad argument"; return SWARM_POLICY_ERR_INVALID; }
    if (in_bf16 && (p->in_dim & 7)) { g_policy_error = "swarm_policy_forward_bf16: in_dim must be a multiple of 8"; return SWARM_POLICY_ERR_INVALID; }
    const bool routed = p->route.n_env > 0;
    if (routed && rows != (int64_t)p->route.n_env * p->route.rows_per_env) {       // no silent fall-back to equal groups
        g_policy_error = "swarm_policy_forward: rows " + std::to_string((long long)rows) + " is not the route's n_env * rows_per_env = " +
                         std::to_string(p->route.n_env) + " * " + std::to_string(p->route.rows_per_env) + " = " +
                         std::to_string((long long)p->route.n_env * p->route.rows_per_env) + " (swarm_policy_bank_route)";
        return SWARM_POLICY_ERR_INVALID;
    }
    if (!routed && rows % p->members != 0) {                // a bank: every member owns rows / members whole rows
        g_policy_error = "swarm_policy_forward: rows " + std::to_string((long long)rows) + " is no multiple of the bank's members " + std::to_string(p->members);
        return SWARM_POLICY_ERR_INVALID;
    }
    if (rows == 0) return SWARM_POLICY_OK;
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = "swarm_policy_forward: hipSetDevice failed"; return SWARM_POLICY_ERR_HIP; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool x3 = p->precision == 1, lp = log_pi != nullptr;
    // a route in force: the tile table of this launch's rows per workgroup (policy_wide.h RouteView)
    const int rg = (!p->wide && x3) ? 1 : 0;
    const swarm_wide::RouteView rv = {routed ? reinterpret_cast<const int4 *>(p->route.d_tab.get() + p->route.off_tiles[rg]) : nullptr,
                                      routed ? p->route.d_tab.get() + p->route.off_order : nullptr, p->route.rows_per_env};
    const unsigned route_grid = routed ? p->route.grid(rg, p->members) : 0u;    // one workgroup per entry of that table
    // the exploration epilogue's parameters, the same for both geometries: the clamped scale, the key of (seed, step), and
    // log-pi's constant act_dim * log(noise_scale * sqrt(2 pi)), in double from the fp32 scale the kernel uses
    // (swarm_policy.h); a kernel without log-pi gets (nullptr, 0.0f)
    const float scale = noise_scale > 0.0f ? noise_scale : 0.0f;
    const unsigned long long noise_key = swarm_noise_key(seed, step);
    const float c = (lp && scale > 0.0f) ? (float)((double)p->act_dim * std::log((double)scale * std::sqrt(2.0 * M_PI))) : 0.0f;
    if (p->wide) {                                          // a wide handle: its own kernels
        const swarm_wide::ForwardArgs a = {obs, in_bf16, rows, act, log_pi, scale, c, noise_key, row_offset, p->precision,
                                           st, !p->smem_set, p->bank, p->members, routed ? &rv : nullptr, route_grid};
        swarm_wide::forward(p->wl, p->d_blob.get(), a);
    } else {
        MlpParams q = p->p;
        q.rows = rows; q.noise_scale = scale; q.noise_key = noise_key; q.row_offset = row_offset;
        if (!p->smem_set) {
            using swarm_wide::raise_smem;
            raise_smem(kPlain, kSmemBytes); raise_smem(kPlainTpw2, kSmemBytes); raise_smem(kBank, kSmemBytes); raise_smem(kRoute, kSmemBytes);
        }
        const int n_waves = waves_of(x3);
        const long long per_block = (long long)n_waves * 32;
        const dim3 b(64 * n_waves);
        if (routed) {                                       // q.rows: the call's
            hipLaunchKernelGGL(kRoute[x3][in_bf16][lp], dim3(route_grid), b, kSmemBytes, st, q, obs, act, log_pi, c, rv);
        } else if (p->bank) {                               // (ceil(R / rows per workgroup), members)
            q.rows = rows / p->members;                     // the kernel's P.rows: the MEMBER's rows
            const dim3 gb((unsigned)((q.rows + per_block - 1) / per_block), (unsigned)p->members);
            hipLaunchKernelGGL(kBank[x3][in_bf16][lp], gb, b, kSmemBytes, st, q, obs, act, log_pi, c);
        } else {
            // one row tile per wave; the two-tile instantiation (SWARM_POLICY_TPW=2, measurement knob, read for a plain narrow
            // handle alone) is slower: 98 vs 87 us on 262144 bf16 rows, 118 vs 106 us on fp32 rows -- one wave per SIMD costs
            // more than the halved LDS reads give back
            const char *ev = std::getenv("SWARM_POLICY_TPW");
            const int tpw = (ev && ev[0] == '2' && !x3) ? 2 : 1;
            const dim3 g((unsigned)((rows + per_block * tpw - 1) / (per_block * tpw)));
            hipLaunchKernelGGL(tpw == 2 ? kPlainTpw2[in_bf16][lp] : kPlain[x3][in_bf16][lp], g, b, kSmemBytes, st, q, obs, act, log_pi, c);
        }
    }
    p->smem_set = true;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_policy_error = std::string("swarm_policy_forward: ") + hipGetErrorString(e); return SWARM_POLICY_ERR_HIP; }
    return SWARM_POLICY_OK;
}

int swarm_policy_set_precision(swarm_policy_t *p, int precision)
{
    if (!p || (precision != SWARM_POLICY_BF16 && precision != SWARM_POLICY_BF16X3)) { g_policy_error = "swarm_policy_set_precision: bad argument"; return SWARM_POLICY_ERR_INVALID; }
    p->precision = precision;
    return SWARM_POLICY_OK;
}

int swarm_policy_forward(swarm_policy_t *p, const float *obs, int64_t rows, float *act, void *stream)
{
    return policy_forward(p, obs, false, rows, act, stream);
}

int swarm_policy_forward_bf16(swarm_policy_t *p, const void *obs_bf16, int64_t rows, float *act, void *stream)
{
    return policy_forward(p, obs_bf16, true, rows, act, stream);
}

int swarm_policy_forward_explore(swarm_policy_t *p, const void *obs, int obs_is_bf16, int64_t rows, float *act,
                                 float noise_scale, uint64_t seed, uint64_t step, void *stream)
{
    return policy_forward(p, obs, obs_is_bf16 != 0, rows, act, stream, noise_scale, seed, step);
}

int swarm_policy_forward_explore_at(swarm_policy_t *p, const void *obs, int obs_is_bf16, int64_t rows, float *act,
                                    float noise_scale, uint64_t seed, uint64_t step, uint64_t row_offset, void *stream)
{
    return policy_forward(p, obs, obs_is_bf16 != 0, rows, act, stream, noise_scale, seed, step, row_offset);
}

int swarm_policy_forward_explore_logpi(swarm_policy_t *p, const void *obs, int obs_is_bf16, int64_t rows, float *act, float *log_pi,
                                      float noise_scale, uint64_t seed, uint64_t step, uint64_t row_offset, void *stream)
{
    if (!log_pi) { g_policy_error = "swarm_policy_forward_explore_logpi: null log_pi (a [rows] fp32 device array is required)"; return SWARM_POLICY_ERR_INVALID; }
    return policy_forward(p, obs, obs_is_bf16 != 0, rows, act, stream, noise_scale, seed, step, row_offset, log_pi);
}

int swarm_policy_load_device(swarm_policy_t *p, const float *w1, const float *b1, const float *w2, const float *b2,
                             const float *w3, const float *b3, const float *w4, const float *b4, void *stream)
{
    if (!p) { g_policy_error = "swarm_policy_load_device: null handle"; return SWARM_POLICY_ERR_INVALID; }
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) { g_policy_error = "swarm_policy_load_device: null weight pointer"; return SWARM_POLICY_ERR_INVALID; }
    if (p->members > 1) {
        g_policy_error = "swarm_policy_load_device: the handle is a bank of " + std::to_string(p->members) + " members (swarm_policy_bank_load_device loads one of them)";
        return SWARM_POLICY_ERR_INVALID;
    }
    const float *const w[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    return load_member("swarm_policy_load_device", p, 0, w, stream);
}

int swarm_policy_bank_load_device(swarm_policy_t *p, int member, const float *w1, const float *b1, const float *w2, const float *b2,
                                  const float *w3, const float *b3, const float *w4, const float *b4, void *stream)
{
    if (!p) { g_policy_error = "swarm_policy_bank_load_device: null handle"; return SWARM_POLICY_ERR_INVALID; }
    if (member < 0 || member >= p->members) {
        g_policy_error = "swarm_policy_bank_load_device: member " + std::to_string(member) + " outside [0, " + std::to_string(p->members) + ")";
        return SWARM_POLICY_ERR_INVALID;
    }
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) { g_policy_error = "swarm_policy_bank_load_device: null weight pointer"; return SWARM_POLICY_ERR_INVALID; }
    const float *const w[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    return load_member("swarm_policy_bank_load_device", p, member, w, stream);
}

int swarm_policy_bank_route(swarm_policy_t *p, const int32_t *member_of_env, int32_t n_env, int32_t rows_per_env, void *stream)
{
    const char *who = "swarm_policy_bank_route: ";
    if (n_env < 0) { g_policy_error = std::string(who) + "n_env " + std::to_string(n_env) + " < 0"; return SWARM_POLICY_ERR_INVALID; }
    if (n_env > 0 && !member_of_env) { g_policy_error = std::string(who) + "null member_of_env with n_env " + std::to_string(n_env); return SWARM_POLICY_ERR_INVALID; }
    if (n_env == 0 && member_of_env) { g_policy_error = std::string(who) + "n_env 0 with a table (a NULL table with n_env 0 ends the route)"; return SWARM_POLICY_ERR_INVALID; }
    if (n_env > 0 && rows_per_env < 1) { g_policy_error = std::string(who) + "rows_per_env " + std::to_string(rows_per_env) + " < 1"; return SWARM_POLICY_ERR_INVALID; }
    const long long rows = (long long)n_env * rows_per_env;
    if (n_env > 0 && rows >= (1ll << 31)) {
        g_policy_error = std::string(who) + "n_env * rows_per_env = " + std::to_string(n_env) + " * " + std::to_string(rows_per_env) + " reaches 2^31 rows";
        return SWARM_POLICY_ERR_INVALID;
    }
    // (the arguments first, then the handle: every refusal above is decided without one)
    if (!p) { g_policy_error = std::string(who) + "null handle"; return SWARM_POLICY_ERR_INVALID; }
    if (!p->bank) { g_policy_error = std::string(who) + "the handle is no bank (swarm_policy_bank_create makes one; a plain handle has one actor for every row)"; return SWARM_POLICY_ERR_INVALID; }
    if (n_env == 0) { p->route.n_env = 0; p->route.rows_per_env = 0; return SWARM_POLICY_OK; }     // equal contiguous groups again
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = std::string(who) + "hipSetDevice failed"; return SWARM_POLICY_ERR_HIP; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    swarm_policy::Route &r = p->route;
    if (rows > r.cap_rows) {                                // the first route, or a larger one than any before: new tables
        // forwards in flight on `stream` read the old ones: wait for them before the allocation is replaced
        hipError_t e = r.d_tab ? hipStreamSynchronize(st) : hipSuccess;
        const int t0 = p->wide ? swarm_wide::kRouteRows : 32 * waves_of(false), t1 = p->wide ? 0 : 32 * waves_of(true);
        const auto up4 = [](size_t v) { return (v + 3) & ~(size_t)3; };             // tile entries are 16-byte loads
        // env_order gets `rows` words although n_env are used: the contract ties allocation to rows alone (a later route over
        // no more rows allocates nothing, whatever its n_env), and n_env <= rows is the only bound rows gives
        const size_t off_order = up4(SWARM_POLICY_BANK_MAX + 1), off_t0 = off_order + up4((size_t)rows);
        const size_t off_t1 = off_t0 + 4 * ((size_t)(rows / t0) + p->members);
        const size_t words = off_t1 + (t1 ? 4 * ((size_t)(rows / t1) + p->members) : 0);
        if (e == hipSuccess) e = r.d_tab.alloc(words);
        if (e != hipSuccess) {
            r.n_env = 0; r.rows_per_env = 0; r.cap_rows = 0;
            g_policy_error = std::string(who) + "allocating the tables: " + hipGetErrorString(e);
            return SWARM_POLICY_ERR_HIP;
        }
        r.cap_rows = rows; r.off_order = off_order; r.off_tiles[0] = off_t0; r.off_tiles[1] = off_t1; r.t_rows[0] = t0; r.t_rows[1] = t1;
    }
    r.n_env = n_env; r.rows_per_env = rows_per_env;
    RouteTableParams q;
    q.member_of_env = member_of_env; q.counts = r.d_tab.get(); q.env_order = r.d_tab.get() + r.off_order;
    for (int g = 0; g < 2; ++g) {
        q.tiles[g] = reinterpret_cast<int4 *>(r.d_tab.get() + r.off_tiles[g]);
        q.t_rows[g] = r.t_rows[g];
        q.n_tiles[g] = r.t_rows[g] ? (int)r.grid(g, p->members) : 0;
    }
    q.n_env = n_env; q.rows_per_env = rows_per_env; q.members = p->members;
    hipLaunchKernelGGL(k_policy_route_table<kRouteThreads>, dim3(1), dim3(kRouteThreads), 0, st, q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { r.n_env = 0; r.rows_per_env = 0; g_policy_error = std::string(who) + hipGetErrorString(e); return SWARM_POLICY_ERR_HIP; }
    return SWARM_POLICY_OK;
}

int swarm_policy_bank_route_read(swarm_policy_t *p, int32_t *counts, int32_t *unserved, int32_t *env_order, void *stream)
{
    const char *who = "swarm_policy_bank_route_read: ";
    if (!p) { g_policy_error = std::string(who) + "null handle"; return -SWARM_POLICY_ERR_INVALID; }
    const swarm_policy::Route &r = p->route;
    if (r.n_env == 0) return 0;
    if (!counts || !unserved) { g_policy_error = std::string(who) + "null counts / unserved"; return -SWARM_POLICY_ERR_INVALID; }
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = std::string(who) + "hipSetDevice failed"; return -SWARM_POLICY_ERR_HIP; }
    hipStream_t st = static_cast<hipStream_t>(stream);      // the copies on the stream, behind the route enqueued there; then the wait
    int32_t head[SWARM_POLICY_BANK_MAX + 1];
    hipError_t e = hipMemcpyAsync(head, r.d_tab.get(), sizeof head, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    long long served = 0;
    if (e == hipSuccess) {
        for (int m = 0; m < p->members; ++m) { counts[m] = head[m]; served += head[m]; }
        *unserved = head[SWARM_POLICY_BANK_MAX];
        if (env_order) {                                    // the served envs, then -1 up to n_env
            if (served > r.n_env) served = r.n_env;
            for (long long i = served; i < r.n_env; ++i) env_order[i] = -1;
            if (served > 0) e = hipMemcpyAsync(env_order, r.d_tab.get() + r.off_order, (size_t)served * sizeof(int32_t), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
    }
    if (e != hipSuccess) { g_policy_error = std::string(who) + hipGetErrorString(e); return -SWARM_POLICY_ERR_HIP; }
    return r.n_env;
}

int64_t swarm_policy_read_packed(swarm_policy_t *p, void *host_dst, int64_t capacity, void *stream)
{
    if (!p) { g_policy_error = "swarm_policy_read_packed: null handle"; return -SWARM_POLICY_ERR_INVALID; }
    if (capacity < 0) { g_policy_error = "swarm_policy_read_packed: negative capacity"; return -SWARM_POLICY_ERR_INVALID; }
    if (p->members > 1) {
        g_policy_error = "swarm_policy_read_packed: the handle is a bank of " + std::to_string(p->members) + " members (swarm_policy_bank_read_packed reads one of them)";
        return -SWARM_POLICY_ERR_INVALID;
    }
    return read_member("swarm_policy_read_packed", p, 0, host_dst, capacity, stream);
}

int64_t swarm_policy_bank_read_packed(swarm_policy_t *p, int member, void *host_dst, int64_t capacity, void *stream)
{
    if (!p) { g_policy_error = "swarm_policy_bank_read_packed: null handle"; return -SWARM_POLICY_ERR_INVALID; }
    if (member < 0 || member >= p->members) {
        g_policy_error = "swarm_policy_bank_read_packed: member " + std::to_string(member) + " outside [0, " + std::to_string(p->members) + ")";
        return -SWARM_POLICY_ERR_INVALID;
    }
    if (capacity < 0) { g_policy_error = "swarm_policy_bank_read_packed: negative capacity"; return -SWARM_POLICY_ERR_INVALID; }
    return read_member("swarm_policy_bank_read_packed", p, member, host_dst, capacity, stream);
}

}  // extern "C"
