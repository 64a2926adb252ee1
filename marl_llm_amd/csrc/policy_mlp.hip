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
// The kernel itself is csrc/policy_mlp_kernel.h, compiled twice: k_policy_mlp for a plain handle, k_policy_mlp_bank for an
// actor bank (BANK: blockIdx.y is the member; swarm_policy_bank_create) -- that file says why it is text and not a template.
constexpr size_t kMemberPieces = ((3 * kMT * kKS + kKS) * 64 * 2 * 16 + (3 * kKP + 32) * 4) / 16;   // a member's blob: high, low, biases
#define POLICY_MLP_KERNEL k_policy_mlp
#define POLICY_MLP_BANK false
#include "policy_mlp_kernel.h"
#undef POLICY_MLP_KERNEL
#undef POLICY_MLP_BANK
#define POLICY_MLP_KERNEL k_policy_mlp_bank
#define POLICY_MLP_BANK true
#include "policy_mlp_kernel.h"
#undef POLICY_MLP_KERNEL
#undef POLICY_MLP_BANK

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

// (A template, launched through launch_pack at the end of the file, only so that the compiler emits it behind the
// k_policy_mlp instantiations: their code, local labels included, stays what it was -- tools/isa_diff.py.)
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

uint16_t bf16_rne(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

thread_local std::string g_policy_error;

// The instantiations a (precision, TPW) choice launches, with and without log-pi.
template <bool IN_BF16, int TPW, bool X3>
void launch_policy(const dim3 &g, const dim3 &b, hipStream_t st, const MlpParams &q, const void *obs, float *act, float *log_pi,
                   float logpi_c)
{
    if (log_pi) hipLaunchKernelGGL((k_policy_mlp<IN_BF16, TPW, X3, true>), g, b, kSmemBytes, st, q, obs, act, log_pi, logpi_c);
    else hipLaunchKernelGGL((k_policy_mlp<IN_BF16, TPW, X3, false>), g, b, kSmemBytes, st, q, obs, act, nullptr, 0.0f);
}

template <bool IN_BF16, int TPW, bool X3>
void set_smem()
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_policy_mlp<IN_BF16, TPW, X3, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kSmemBytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_policy_mlp<IN_BF16, TPW, X3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kSmemBytes);
}

template <int THREADS>
void launch_pack(const PackParams &q, hipStream_t st)
{
    const unsigned grid = (kPackPieces + kPackBias + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_policy_pack<THREADS>, dim3(grid), dim3(THREADS), 0, st, q);
}

// The same for a bank handle (behind the plain handle's templates, so that their instantiations come first as before).
template <bool IN_BF16, bool X3>
void launch_bank(const dim3 &g, const dim3 &b, hipStream_t st, const MlpParams &q, const void *obs, float *act, float *log_pi, float logpi_c)
{
    if (log_pi) hipLaunchKernelGGL((k_policy_mlp_bank<IN_BF16, 1, X3, true>), g, b, kSmemBytes, st, q, obs, act, log_pi, logpi_c);
    else hipLaunchKernelGGL((k_policy_mlp_bank<IN_BF16, 1, X3, false>), g, b, kSmemBytes, st, q, obs, act, nullptr, 0.0f);
}

template <bool IN_BF16, bool X3>
void set_smem_bank()
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_policy_mlp_bank<IN_BF16, 1, X3, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kSmemBytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_policy_mlp_bank<IN_BF16, 1, X3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kSmemBytes);
}

// The blob of one actor as swarm_policy_create uploads it (and a bank holds once per member): [w1 | w2 | w3 | w4] fragments
// (8 bf16 per lane), their low parts in the same layout, then [b1 | b2 | b3 | b4] fp32.
constexpr size_t kFrag = 64 * 8;                                              // bf16 elements per fragment
constexpr size_t kHidElems = (size_t)kMT * kKS * kFrag, kOutElems = (size_t)kKS * kFrag;
constexpr size_t kWElems = 3 * kHidElems + kOutElems;
constexpr size_t kBlobBytes = 2 * kWElems * 2 + (3 * kKP + 32) * 4;           // high parts, low parts, biases
static_assert(kBlobBytes == kMemberPieces * 16 && kWElems / 8 == (size_t)kPackPieces && kPackBias == 3 * kKP + 32, "a member's blob is whole pieces");

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
    swarm_internal::DevBuf<unsigned char> d_blob;     // the packed weights and biases p points into
    size_t blob_bytes = 0;
    MlpParams p;
    bool smem_set = false;
    swarm_wide::Handle *wide = nullptr;    // swarm_policy_create_wide: the handle runs csrc/policy_wide.hip; d_blob and p stay empty
    // swarm_policy_bank_create: `members` blobs of blob_bytes each, one behind the other (d_blob, or the wide handle's); p points
    // into the first.  A bank handle runs the BANK kernels, also with one member.
    bool bank = false;
    int members = 1;
    ~swarm_policy() { swarm_wide::destroy(wide); }
};

int swarm_internal_policy_info(const swarm_policy_t *p, swarm_policy_info *out)
{
    if (!p || !out) return SWARM_POLICY_ERR_INVALID;
    out->device = p->device; out->in_dim = p->in_dim; out->act_dim = p->act_dim; out->members = p->members;
    return SWARM_POLICY_OK;
}

namespace {

// The packing launch of swarm_policy_load_device / swarm_policy_bank_load_device: member `member`'s slice of the blob.
int load_member(const char *who, swarm_policy_t *p, int member, const float *const w[8], void *stream)
{
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = std::string(who) + ": hipSetDevice failed"; return SWARM_POLICY_ERR_HIP; }
    if (p->wide) {
        const int rc = swarm_wide::load_device(p->wide, member, w, static_cast<hipStream_t>(stream), g_policy_error);
        if (rc != SWARM_POLICY_OK) g_policy_error = std::string(who) + ": " + g_policy_error;
        return rc;
    }
    static_assert(kPackPieces % 64 == 0 && sizeof(bf8) == sizeof(uint4), "one 16-byte piece per fragment lane");
    PackParams q;
    q.w1 = w[0]; q.b1 = w[1]; q.w2 = w[2]; q.b2 = w[3]; q.w3 = w[4]; q.b3 = w[5]; q.w4 = w[6]; q.b4 = w[7];
    q.hi = reinterpret_cast<uint4 *>(p->d_blob.get() + (size_t)member * p->blob_bytes);
    q.lo = q.hi + kPackPieces;
    q.bias = reinterpret_cast<float *>(q.lo + kPackPieces);
    q.in_dim = p->in_dim; q.hidden = p->hidden; q.act_dim = p->act_dim;
    launch_pack<kPackThreads>(q, static_cast<hipStream_t>(stream));
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
    size_t unused;
    const unsigned char *src = p->wide ? static_cast<const unsigned char *>(swarm_wide::blob(p->wide, &unused)) : p->d_blob.get();
    hipError_t e = hipMemcpyAsync(host_dst, src + (size_t)member * p->blob_bytes, p->blob_bytes, hipMemcpyDeviceToHost, st);
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
    if (in_dim < 4 || in_dim > kKP || (in_dim & 3) || hidden < 1 || hidden >= kKP || act_dim < 1 || act_dim > 4) {
        g_policy_error = "swarm_policy_create: supported shapes are in_dim <= 192 (multiple of 4), hidden <= 191, act_dim <= 4";
        return SWARM_POLICY_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_policy_error = "swarm_policy_create: no HIP device (there is no CPU path)"; return SWARM_POLICY_ERR_HIP; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    const DeviceGuard guard(device < ndev ? device : -1);       // -1 is no device: !ok
    if (!guard.ok) { g_policy_error = "swarm_policy_create: bad device"; return SWARM_POLICY_ERR_HIP; }

    const float *const w[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    const std::vector<unsigned char> blob = pack_host(w, in_dim, hidden, act_dim);
    const size_t bytes = blob.size();

    swarm_policy *p = new (std::nothrow) swarm_policy;
    if (!p) return SWARM_POLICY_ERR_INVALID;
    p->device = device; p->in_dim = in_dim; p->hidden = hidden; p->act_dim = act_dim; p->blob_bytes = bytes;
    if (p->d_blob.alloc(bytes) != hipSuccess || hipMemcpy(p->d_blob.get(), blob.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        delete p;
        g_policy_error = "swarm_policy_create: device allocation / upload failed";
        return SWARM_POLICY_ERR_HIP;
    }
    point_params(p->p, p->d_blob.get(), in_dim, act_dim);
    *out = p;
    return SWARM_POLICY_OK;
}

int swarm_policy_create_wide(const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3,
                             const float *w4, const float *b4, int in_dim, int hidden, int act_dim, int device, swarm_policy_t **out)
{
    if (!out) return SWARM_POLICY_ERR_INVALID;
    *out = nullptr;
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4) { g_policy_error = "swarm_policy_create_wide: null weight pointer"; return SWARM_POLICY_ERR_INVALID; }
    if (!swarm_wide::shape_ok(in_dim, hidden, act_dim)) {
        g_policy_error = "swarm_policy_create_wide: supported shapes are in_dim <= 384 (multiple of 4), hidden <= 256, act_dim <= 4";
        return SWARM_POLICY_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_policy_error = "swarm_policy_create_wide: no HIP device (there is no CPU path)"; return SWARM_POLICY_ERR_HIP; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    const DeviceGuard guard(device < ndev ? device : -1);       // -1 is no device: !ok
    if (!guard.ok) { g_policy_error = "swarm_policy_create_wide: bad device"; return SWARM_POLICY_ERR_HIP; }
    swarm_policy *p = new (std::nothrow) swarm_policy;
    if (!p) return SWARM_POLICY_ERR_INVALID;
    p->device = device; p->in_dim = in_dim; p->hidden = hidden; p->act_dim = act_dim;
    const float *const w[8] = {w1, b1, w2, b2, w3, b3, w4, b4};
    const int rc = swarm_wide::create(w, 1, in_dim, hidden, act_dim, &p->wide, g_policy_error);
    if (rc != SWARM_POLICY_OK) { delete p; g_policy_error = "swarm_policy_create_wide: " + g_policy_error; return rc; }
    (void)swarm_wide::blob(p->wide, &p->blob_bytes);
    *out = p;
    return SWARM_POLICY_OK;
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
    if (wide ? !swarm_wide::shape_ok(in_dim, hidden, act_dim) : !narrow_shape_ok(in_dim, hidden, act_dim)) {
        g_policy_error = wide ? "swarm_policy_bank_create: supported shapes of the wide geometry are in_dim <= 384 (multiple of 4), hidden <= 256, act_dim <= 4"
                              : "swarm_policy_bank_create: supported shapes of the narrow geometry are in_dim <= 192 (multiple of 4), hidden <= 191, act_dim <= 4";
        return SWARM_POLICY_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_policy_error = "swarm_policy_bank_create: no HIP device (there is no CPU path)"; return SWARM_POLICY_ERR_HIP; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    const DeviceGuard guard(device < ndev ? device : -1);       // -1 is no device: !ok
    if (!guard.ok) { g_policy_error = "swarm_policy_bank_create: bad device"; return SWARM_POLICY_ERR_HIP; }
    swarm_policy *p = new (std::nothrow) swarm_policy;
    if (!p) { g_policy_error = "swarm_policy_bank_create: out of memory"; return SWARM_POLICY_ERR_INVALID; }
    p->device = device; p->in_dim = in_dim; p->hidden = hidden; p->act_dim = act_dim; p->bank = true; p->members = members;
    if (wide) {
        const int rc = swarm_wide::create(w, members, in_dim, hidden, act_dim, &p->wide, g_policy_error);
        if (rc != SWARM_POLICY_OK) { delete p; g_policy_error = "swarm_policy_bank_create: " + g_policy_error; return rc; }
        (void)swarm_wide::blob(p->wide, &p->blob_bytes);
        *out = p;
        return SWARM_POLICY_OK;
    }
    // every member's slice is the blob swarm_policy_create builds from the same arrays: the same packer, M times
    std::vector<unsigned char> blob;
    blob.reserve((size_t)members * kBlobBytes);
    for (int m = 0; m < members; ++m) {
        const std::vector<unsigned char> one = pack_host(w + 8 * m, in_dim, hidden, act_dim);
        blob.insert(blob.end(), one.begin(), one.end());
    }
    p->blob_bytes = kBlobBytes;
    // the upload on a stream of its own, waited for here: no null-stream work, complete on return
    hipStream_t up = nullptr;
    hipError_t e = p->d_blob.alloc(blob.size());
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);
    if (up) (void)hipStreamDestroy(up);
    if (e != hipSuccess) {
        delete p;
        g_policy_error = "swarm_policy_bank_create: device allocation / upload failed";
        return SWARM_POLICY_ERR_HIP;
    }
    point_params(p->p, p->d_blob.get(), in_dim, act_dim);
    *out = p;
    return SWARM_POLICY_OK;
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
    if (rows % p->members != 0) {                           // a bank: every member owns rows / members whole rows
        g_policy_error = "swarm_policy_forward: rows " + std::to_string((long long)rows) + " is no multiple of the bank's members " + std::to_string(p->members);
        return SWARM_POLICY_ERR_INVALID;
    }
    if (rows == 0) return SWARM_POLICY_OK;
    const DeviceGuard guard(p->device);
    if (!guard.ok) { g_policy_error = "swarm_policy_forward: hipSetDevice failed"; return SWARM_POLICY_ERR_HIP; }
    if (p->wide) {                                          // a wide handle: its own kernel, SWARM_POLICY_TPW not read
        const swarm_wide::ForwardArgs a = {obs, in_bf16, rows, act, log_pi, noise_scale, seed, step, row_offset, p->precision,
                                           static_cast<hipStream_t>(stream), p->bank};
        return swarm_wide::forward(p->wide, a, g_policy_error);
    }
    MlpParams q = p->p;
    q.rows = rows;
    q.noise_scale = noise_scale > 0.0f ? noise_scale : 0.0f;
    q.noise_key = swarm_noise_key(seed, step);
    q.row_offset = row_offset;
    // log-pi's constant act_dim * log(noise_scale * sqrt(2 pi)), in double from the fp32 scale the kernel uses (swarm_policy.h)
    const float logpi_c = q.noise_scale > 0.0f ? (float)((double)p->act_dim * std::log((double)q.noise_scale * std::sqrt(2.0 * M_PI))) : 0.0f;
    // one row tile per wave; the two-tile instantiation (SWARM_POLICY_TPW=2, measurement knob) is slower: 98 vs 87 us on
    // 262144 bf16 rows, 118 vs 106 us on fp32 rows -- one wave per SIMD costs more than the halved LDS reads give back
    int tpw = 1;
    if (const char *ev = std::getenv("SWARM_POLICY_TPW")) tpw = ev[0] == '2' ? 2 : 1;
    if (p->precision == 1) tpw = 1;
    const int n_waves = waves_of(p->precision == 1);
    const long long per_block = (long long)n_waves * 32 * tpw;
    const unsigned grid = (unsigned)((rows + per_block - 1) / per_block);
    if (!p->smem_set) {
        set_smem<false, 1, false>(); set_smem<true, 1, false>();
        set_smem<false, 2, false>(); set_smem<true, 2, false>();
        set_smem<false, 1, true>(); set_smem<true, 1, true>();
        set_smem_bank<false, false>(); set_smem_bank<true, false>(); set_smem_bank<false, true>(); set_smem_bank<true, true>();
        p->smem_set = true;
    }
    const dim3 g(grid), b(64 * n_waves);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p->bank) {                                          // (ceil(R / rows per workgroup), members); SWARM_POLICY_TPW not read
        q.rows = rows / p->members;                         // the kernel's P.rows: the MEMBER's rows
        const long long bank_block = (long long)n_waves * 32;
        const dim3 gb((unsigned)((q.rows + bank_block - 1) / bank_block), (unsigned)p->members);
        if (p->precision == 1) {
            if (in_bf16) launch_bank<true, true>(gb, b, st, q, obs, act, log_pi, logpi_c);
            else launch_bank<false, true>(gb, b, st, q, obs, act, log_pi, logpi_c);
        } else {
            if (in_bf16) launch_bank<true, false>(gb, b, st, q, obs, act, log_pi, logpi_c);
            else launch_bank<false, false>(gb, b, st, q, obs, act, log_pi, logpi_c);
        }
    } else if (p->precision == 1) {
        if (in_bf16) launch_policy<true, 1, true>(g, b, st, q, obs, act, log_pi, logpi_c);
        else launch_policy<false, 1, true>(g, b, st, q, obs, act, log_pi, logpi_c);
    } else if (tpw == 2) {
        if (in_bf16) launch_policy<true, 2, false>(g, b, st, q, obs, act, log_pi, logpi_c);
        else launch_policy<false, 2, false>(g, b, st, q, obs, act, log_pi, logpi_c);
    } else {
        if (in_bf16) launch_policy<true, 1, false>(g, b, st, q, obs, act, log_pi, logpi_c);
        else launch_policy<false, 1, false>(g, b, st, q, obs, act, log_pi, logpi_c);
    }
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
