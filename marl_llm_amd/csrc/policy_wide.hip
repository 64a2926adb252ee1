// The fused actor's WIDE geometry: the kernel of policy_mlp.hip for observation rows up to 384 wide and hidden widths up to
// 256 (num_obs_grid_max up to 176 at the default topology, --hidden_dim up to 256).  Same scheme -- bf16
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation, every layer transposed (H^T = W . X^T, a wavefront's 32 rows on the
// lanes), the accumulator tile of layer l the B operand of layer l + 1, no activation ever leaves the registers, the weights
// stream through a double-buffered LDS ring -- with three differences:
//
// 1. The weight stream is cut along K, not along the features: a chunk is ALL MT feature tiles x 4 k-steps (MT = 8: 32
//    fragments, 32 KB; two buffers + bias tails = 66 KB of LDS).  All accumulators of a layer are live anyway, and layer 1
//    then needs only the 4 B fragments of the current chunk: the observation row is read 64 columns at a time, the next
//    piece in flight while the MFMAs of this one run, so in_dim = 384 (24 k-steps) costs no more registers than in_dim = 64.
//    Layer 1's stream is also only as long as the row: ceil(in_dim / 64) chunks.
// 2. Biases initialise the accumulators (there is no padded feature left for a constant-one column at hidden = 256).  The
//    first chunk of every layer carries the layer's bias as fp32 values behind its fragments: b1 itself, bf(b) for layers
//    2-4; in bf16x3 mode the LOW stream's chunk carries lo(b) = bf(b - bf(b)), added when that chunk arrives -- the terms
//    hi and lo of include/swarm_policy.h, summed in fp32.
// 3. Two padded hidden widths, chosen by the handle: MT = 6 (hidden <= 192) and MT = 8 (hidden <= 256).
//
// A workgroup is four wavefronts = 128 rows at both precisions, one wavefront per SIMD (launch bounds (256, 1): the unified
// 512-register file holds 128 accumulators + 64 + 64 packed activation registers + the prefetched chunk without scratch).
// Fragment maps as in policy_mlp.hip: A[row = l & 31][k = 8 (l >> 5) + j], B[k = 8 (l >> 5) + j][col = l & 31], C/D col = l & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  The arithmetic is the contract of include/swarm_policy.h;
// tests/test_gpu_policy_wide.py holds the kernel to the float64 model of it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "policy_wide.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
typedef __attribute__((ext_vector_type(16))) float f16v;

using swarm_internal::pmix64;

constexpr int kWaves = 4;                 // wavefronts (32-row tiles) per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kRowsPerBlock = 32 * kWaves;

// Geometry of one padded hidden width, in 16-byte PIECES (one lane's share of a fragment: 8 bf16, or 4 fp32 of a bias tail).
// Stream: [layer 1: n1 chunks][layer 2: KC][layer 3: KC][output layer: 1], every chunk in a slot of CH pieces:
//   hidden-layer and layer-1 chunk g:   [feature tile mt][k-step 4 g + i][lane]  (W pieces), then the bias tail (TAIL pieces:
//                                        32 MT fp32, live in a layer's first chunk only, zeros elsewhere)
//   output chunk:                       [k-step][lane] of feature tile 0 (WOUT pieces), then the bias tail
template <int MT>
struct Geo {
    static constexpr int KS = 2 * MT;                 // k-steps of a hidden layer
    static constexpr int KC = MT / 2;                 // chunks of a hidden layer (4 k-steps each)
    static constexpr int W = MT * 4 * 64;
    static constexpr int TAIL = MT * 8;
    static constexpr int CH = W + TAIL;
    static constexpr int WOUT = KS * 64;
    static constexpr int PRE = (CH + kThreads - 1) / kThreads;
    static constexpr int SMEM = 2 * CH * 16;
};

// the raw values of one layer-1 chunk of a lane's row: 2 x 4 fp32 or 8 bf16 for each of the 4 k-steps
template <bool IN_BF16>
struct XRaw {
    float4 f[IN_BF16 ? 1 : 4][2];
    bf8 b[IN_BF16 ? 4 : 1];
};

struct WideParams {
    const bf8 *hi, *lo;                // the high and the low stream
    int in_dim, act_dim;
    long long rows;
    float noise_scale;                 // the exploration epilogue: as MlpParams of policy_mlp.hip
    unsigned long long noise_key, row_offset;
};

// tanh, exploration noise, clamp and log-pi of one row: the generator and the formulas of include/swarm_policy.h, the
// statements of k_policy_mlp's epilogue (the two kernels give the same bits for the same pre-tanh values)
template <bool LOGPI>
__device__ __forceinline__ void finish_row(const WideParams &P, const f16v &o, long long row, float *__restrict__ act,
                                           float *__restrict__ log_pi, float logpi_c)
{
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
            float v = tanhf(o[k]);
            if (P.noise_scale > 0.0f) v = fminf(fmaxf(v + P.noise_scale * z[k], -1.0f), 1.0f);
            y[k] = v;
        }
    if constexpr (LOGPI) {                                  // -(0.5 sum_k z_k^2) - c, the sum in k order
        float lp = -0.0f;
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

// The kernel itself is csrc/policy_wide_kernel.h, compiled three times: for a plain handle, for an actor bank (BANK) and for
// a bank under a route (ROUTE: swarm_policy_bank_route).
#define POLICY_WIDE_KERNEL k_policy_wide
#define POLICY_WIDE_BANK false
#define POLICY_WIDE_ROUTE 0
#include "policy_wide_kernel.h"
#undef POLICY_WIDE_KERNEL
#undef POLICY_WIDE_BANK
#define POLICY_WIDE_KERNEL k_policy_wide_bank
#define POLICY_WIDE_BANK true
#include "policy_wide_kernel.h"
#undef POLICY_WIDE_KERNEL
#undef POLICY_WIDE_BANK
#undef POLICY_WIDE_ROUTE
#define POLICY_WIDE_KERNEL k_policy_wide_route
#define POLICY_WIDE_BANK false
#define POLICY_WIDE_ROUTE 1
#include "policy_wide_kernel.h"
#undef POLICY_WIDE_KERNEL
#undef POLICY_WIDE_BANK
#undef POLICY_WIDE_ROUTE
static_assert(kRowsPerBlock == swarm_wide::kRouteRows, "the route's tile table is cut for this workgroup");

// ---- the packed stream, on the host (pack_host) and on the device (load_device): the two are written independently and
// tests/test_gpu_policy_wide.py compares their bytes.
using swarm_wide::Layout;

struct PackParams {
    const float *w[8];                 // fc1.weight, fc1.bias, ..., fc4.bias, device
    uint4 *hi, *lo;                    // the two streams, n_chunks * ch pieces each
    Layout g;
};

// round-to-nearest-even on the bit pattern (integer: no conversion's denormal mode to trust)
__host__ __device__ inline unsigned rne_bf16(unsigned u)
{
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (u >> 16) | 0x40u;     // NaN (outside the contract)
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}

// One thread per piece of a stream: the piece's 8 weights as high and low bf16 parts, or 4 bias values of a layer's first
// chunk (fp32: b1 | 0 for layer 1, bf(b) | bf(b - bf(b)) for the others), or the zeros of a slot's unused pieces.
__global__ void __launch_bounds__(256) k_policy_wide_pack(const PackParams P)
{
    const Layout &g = P.g;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= g.n_chunks * g.ch) return;
    const int c = q / g.ch, rp = q - c * g.ch;
    int layer, kg;                                                          // chunk c = k-group kg of layer 0..3
    if (c < g.n1) { layer = 0; kg = c; }
    else if (c < g.n1 + g.kc) { layer = 1; kg = c - g.n1; }
    else if (c < g.n1 + 2 * g.kc) { layer = 2; kg = c - g.n1 - g.kc; }
    else { layer = 3; kg = 0; }
    const float *__restrict__ wm = P.w[2 * layer], *__restrict__ bv = P.w[2 * layer + 1];
    const int n_out = layer == 3 ? g.act_dim : g.hidden, n_in = layer == 0 ? g.in_dim : g.hidden;
    const int n_w = layer == 3 ? g.wout : g.w;
    unsigned hv[8], lv[8];
    if (rp < n_w) {
        const int lane = rp & 63, hh = lane >> 5;
        const int mt = layer == 3 ? 0 : rp >> 8, ks = layer == 3 ? rp >> 6 : 4 * kg + ((rp >> 6) & 3);
        const int o = 32 * mt + (lane & 31);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // natural k order where B comes from memory, the accumulator tile's order elsewhere
            const int k = layer == 0 ? 16 * ks + 8 * hh + j : 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * hh + (j & 3);
            const float v = (o < n_out && k < n_in) ? wm[(size_t)o * n_in + k] : 0.0f;
            hv[j] = rne_bf16(__float_as_uint(v));
            lv[j] = rne_bf16(__float_as_uint(v - __uint_as_float(hv[j] << 16)));      // the IEEE fp32 difference, denormals kept
        }
        P.hi[q] = make_uint4(hv[0] | hv[1] << 16, hv[2] | hv[3] << 16, hv[4] | hv[5] << 16, hv[6] | hv[7] << 16);
        P.lo[q] = make_uint4(lv[0] | lv[1] << 16, lv[2] | lv[3] << 16, lv[4] | lv[5] << 16, lv[6] | lv[7] << 16);
        return;
    }
    unsigned th[4] = {0u, 0u, 0u, 0u}, tl[4] = {0u, 0u, 0u, 0u};
    const int t = rp - n_w;
    if (kg == 0 && t < g.tail) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int f = 4 * t + e;
            if (f < n_out) {
                const unsigned u = __float_as_uint(bv[f]);
                if (layer == 0) th[e] = u;
                else {
                    th[e] = rne_bf16(u) << 16;
                    tl[e] = rne_bf16(__float_as_uint(bv[f] - __uint_as_float(th[e]))) << 16;
                }
            }
        }
    }
    P.hi[q] = make_uint4(th[0], th[1], th[2], th[3]);
    P.lo[q] = make_uint4(tl[0], tl[1], tl[2], tl[3]);
}

float bits_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t float_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// The kernels a forward call chooses from, per kernel text: [mt == 8][x3][in_bf16][log_pi].
using WideKernel = void (*)(WideParams, const void *, float *, float *, float);
using WideRouteKernel = void (*)(WideParams, const void *, float *, float *, float, swarm_wide::RouteView);
#define WIDE_KERNELS(K, X3, MT) {{K<false, X3, false, MT>, K<false, X3, true, MT>}, {K<true, X3, false, MT>, K<true, X3, true, MT>}}
#define WIDE_TABLE(K) {{WIDE_KERNELS(K, false, 6), WIDE_KERNELS(K, true, 6)}, {WIDE_KERNELS(K, false, 8), WIDE_KERNELS(K, true, 8)}}
const WideKernel kPlain[2][2][2][2] = WIDE_TABLE(k_policy_wide), kBank[2][2][2][2] = WIDE_TABLE(k_policy_wide_bank);
const WideRouteKernel kRoute[2][2][2][2] = WIDE_TABLE(k_policy_wide_route);
#undef WIDE_TABLE
#undef WIDE_KERNELS
static_assert(Geo<8>::SMEM <= 160 * 1024 && swarm_wide::kMaxHidden == 32 * 8 && swarm_wide::kMaxIn % 64 == 0, "the widest geometry");

}  // namespace

namespace swarm_wide {

bool shape_ok(int in_dim, int hidden, int act_dim)
{
    return in_dim >= 4 && in_dim <= kMaxIn && !(in_dim & 3) && hidden >= 1 && hidden <= kMaxHidden && act_dim >= 1 && act_dim <= kMaxAct;
}

Layout layout_of(int in_dim, int hidden, int act_dim)
{
    Layout g;
    g.mt = hidden <= 192 ? 6 : 8;
    g.kc = g.mt / 2; g.w = g.mt * 256; g.tail = g.mt * 8; g.ch = g.w + g.tail; g.wout = 2 * g.mt * 64;
    g.n1 = (in_dim + 63) / 64;
    g.n_chunks = g.n1 + 2 * g.kc + 1;
    g.in_dim = in_dim; g.hidden = hidden; g.act_dim = act_dim;
    return g;
}

// The host packer: the stream built layer by layer into a zeroed blob.
std::vector<unsigned char> pack_host(const Layout &g, const float *const w[8])
{
    const size_t stream_elems = (size_t)g.n_chunks * g.ch * 8;              // bf16 elements of one stream
    std::vector<unsigned char> blob(2 * stream_elems * 2, 0);
    uint16_t *hi = reinterpret_cast<uint16_t *>(blob.data()), *lo = hi + stream_elems;
    auto put = [&](size_t piece, int j, float v) {
        const uint16_t hb = (uint16_t)rne_bf16(float_bits(v));
        hi[piece * 8 + j] = hb;
        lo[piece * 8 + j] = (uint16_t)rne_bf16(float_bits(v - bits_float((uint32_t)hb << 16)));
    };
    auto k_acc = [](int ks, int h, int j) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3); };
    auto put_bias = [&](int chunk, int off, const float *b, int n, bool fp32) {
        const size_t at = ((size_t)chunk * g.ch + off) * 16;                // byte offset inside a stream
        unsigned char *th = blob.data() + at, *tl = blob.data() + stream_elems * 2 + at;
        for (int f = 0; f < n; ++f) {
            uint32_t uh = float_bits(b[f]), ul = 0;
            if (!fp32) {
                uh = rne_bf16(uh) << 16;
                ul = rne_bf16(float_bits(b[f] - bits_float(uh))) << 16;
            }
            std::memcpy(th + 4 * f, &uh, 4);
            std::memcpy(tl + 4 * f, &ul, 4);
        }
    };
    for (int c = 0; c < g.n1; ++c)                                          // layer 1: natural k order
        for (int mt = 0; mt < g.mt; ++mt)
            for (int i = 0; i < 4; ++i)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int o = 32 * mt + (lane & 31), k = 16 * (4 * c + i) + 8 * (lane >> 5) + j;
                        const float v = (o < g.hidden && k < g.in_dim) ? w[0][(size_t)o * g.in_dim + k] : 0.0f;
                        put((size_t)c * g.ch + (mt * 4 + i) * 64 + lane, j, v);
                    }
    put_bias(0, g.w, w[1], g.hidden, true);
    for (int l = 0; l < 2; ++l) {                                           // layers 2 and 3
        const int base = g.n1 + l * g.kc;
        for (int kc = 0; kc < g.kc; ++kc)
            for (int mt = 0; mt < g.mt; ++mt)
                for (int i = 0; i < 4; ++i)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int o = 32 * mt + (lane & 31), k = k_acc(4 * kc + i, lane >> 5, j);
                            const float v = (o < g.hidden && k < g.hidden) ? w[2 + 2 * l][(size_t)o * g.hidden + k] : 0.0f;
                            put((size_t)(base + kc) * g.ch + (mt * 4 + i) * 64 + lane, j, v);
                        }
        put_bias(base, g.w, w[3 + 2 * l], g.hidden, false);
    }
    const int c_out = g.n1 + 2 * g.kc;                                      // the output layer: feature tile 0
    for (int ks = 0; ks < 2 * g.mt; ++ks)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int o = lane & 31, k = k_acc(ks, lane >> 5, j);
                const float v = (o < g.act_dim && k < g.hidden) ? w[6][(size_t)o * g.hidden + k] : 0.0f;
                put((size_t)c_out * g.ch + ks * 64 + lane, j, v);
            }
    put_bias(c_out, g.wout, w[7], g.act_dim, false);
    return blob;
}

void forward(const Layout &g, const void *blob, const ForwardArgs &a)
{
    WideParams q;
    q.hi = reinterpret_cast<const bf8 *>(blob);
    q.lo = q.hi + (size_t)g.n_chunks * g.ch;
    q.in_dim = g.in_dim; q.act_dim = g.act_dim; q.rows = a.rows;
    q.noise_scale = a.noise_scale; q.noise_key = a.noise_key; q.row_offset = a.row_offset;
    const auto smem_of = [](int mt8) { return mt8 ? Geo<8>::SMEM : Geo<6>::SMEM; };
    if (a.set_smem)
        for (int m = 0; m < 2; ++m) { raise_smem(kPlain[m], smem_of(m)); raise_smem(kBank[m], smem_of(m)); raise_smem(kRoute[m], smem_of(m)); }
    const int wide8 = g.mt == 8, x3 = a.precision == SWARM_POLICY_BF16X3, lp = a.log_pi != nullptr;
    const unsigned smem = smem_of(wide8);
    const dim3 b(kThreads);
    if (a.route) {                                          // one workgroup per tile-table entry, q.rows the call's rows
        hipLaunchKernelGGL(kRoute[wide8][x3][a.in_bf16][lp], dim3(a.route_grid), b, smem, a.stream, q, a.obs, a.act, a.log_pi, a.logpi_c, *a.route);
        return;
    }
    // a bank handle: grid (ceil(R / 128), members), and the kernel's P.rows is the MEMBER's rows R = rows / members (the caller
    // has checked the division)
    if (a.bank) q.rows = a.rows / a.members;
    const dim3 grid((unsigned)((q.rows + kRowsPerBlock - 1) / kRowsPerBlock), a.bank ? (unsigned)a.members : 1u);
    hipLaunchKernelGGL((a.bank ? kBank : kPlain)[wide8][x3][a.in_bf16][lp], grid, b, smem, a.stream, q, a.obs, a.act, a.log_pi, a.logpi_c);
}

void load_device(const Layout &g, void *dst, const float *const w[8], hipStream_t st)
{
    PackParams q;
    for (int i = 0; i < 8; ++i) q.w[i] = w[i];
    q.hi = static_cast<uint4 *>(dst);
    q.lo = q.hi + (size_t)g.n_chunks * g.ch;
    q.g = g;
    const unsigned grid = (unsigned)((g.n_chunks * g.ch + 255) / 256);
    hipLaunchKernelGGL(k_policy_wide_pack, dim3(grid), dim3(256), 0, st, q);
}

}  // namespace swarm_wide
