// env_large.hip -- the env step of a handle created with swarm_config_t.large_swarm: two small kernels that serve any
// n_agents in [1, 1024], where the step kernel of swarm_env.hip (k_env: one workgroup per env, its state in LDS) ends at 256.
//
// Given the post-integration positions and velocities of its env, everything an agent's step produces -- neighbour list,
// nearest cell, sensed and occupied lists, observation row, reward, the next step's contact force and prior -- depends on no
// other agent's derived result (AssemblyEnv.cpp and assembly.py, function by function).  So a step is two launches on the handle's
// stream, and the kernel boundary between them is the only env-wide barrier:
//   k_large_move     one thread per agent: forces, integration, clip, wrap; p and dp in place (ENV:487-652).
//   k_large_observe  one wavefront per agent, on the new state: the whole of an observation pass.  No workgroup barrier: the
//                    four waves of a workgroup only share the L1 (consecutive agents of one env) and each owns a slice of LDS.
// Every decision is fp64 in the reference's operation order (-ffp-contract=off); the only deviations are the three DESIGN.md
// lists for k_env: neighbours ordered by (norm, index) with self removed by id, nearest cell by squared distance, and the
// reward's cosine as a polynomial.  The device functions are plain restatements: nothing is shared with swarm_env.hip.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "swarm_env.h"
#include "env_types.h"

using namespace swarm_internal;

namespace {

typedef unsigned long long u64;

constexpr int kWaves = 4;        // agents (= wavefronts) per workgroup
constexpr int kNbCap = 256;      // nearby agents staged in LDS per pass of the occupied filter (more: further passes)

template <typename T> struct Pair;
template <> struct Pair<float>  { typedef float2 type; };
template <> struct Pair<double> { typedef double2 type; };
typedef __attribute__((ext_vector_type(2))) __bf16 bf2v;
template <> struct Pair<__bf16> { typedef bf2v type; };
typedef float f2v __attribute__((ext_vector_type(2)));
typedef double d2v __attribute__((ext_vector_type(2)));

// one rounding for f64 / f32; bf16 = the f32 value rounded again
template <typename OT> __device__ __forceinline__ OT to_out(double v) { return (OT)v; }
template <> __device__ __forceinline__ __bf16 to_out<__bf16>(double v) { return (__bf16)(float)v; }
__device__ __forceinline__ void store_nt(float2 *dst, float2 v) { f2v t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<f2v *>(dst)); }
__device__ __forceinline__ void store_nt(double2 *dst, double2 v) { d2v t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<d2v *>(dst)); }
__device__ __forceinline__ void store_nt(bf2v *dst, bf2v v) { __builtin_nontemporal_store(v, dst); }

__device__ __forceinline__ void wrap_rel(double &x, double &y, double wh, double hh)
{   // CPP:700-715
    if (x < -wh) x += 2 * wh; else if (x > wh) x -= 2 * wh;
    if (y < -hh) y += 2 * hh; else if (y > hh) y -= 2 * hh;
}

__device__ __forceinline__ double clamp_ref(double v, double lo, double hi)
{   // CPP:11-14  std::max(lo, std::min(v, hi))
    double m = (hi < v) ? hi : v;
    return (lo < m) ? m : lo;
}

// cos(pi * t) for t in [0, 1], absolute error ~2e-16 (Taylor in x = pi * min(t, 1 - t) up to x^22): the reward's psi weight
// (CPP:1012-1020 calls libm's cos), which feeds a sum that is compared with a threshold (DESIGN.md deviation 3)
__device__ __forceinline__ double cospi01(double t)
{
    const bool flip = t > 0.5;
    const double r = flip ? 1.0 - t : t;
    const double x = M_PI * r;
    const double u = x * x;
    double c = -8.8967913924505741e-22;
    c = fma(c, u, 4.1103176233121648e-19);
    c = fma(c, u, -1.5619206968586225e-16);
    c = fma(c, u, 4.7794773323873853e-14);
    c = fma(c, u, -1.1470745597729725e-11);
    c = fma(c, u, 2.0876756987868100e-09);
    c = fma(c, u, -2.7557319223985888e-07);
    c = fma(c, u, 2.4801587301587302e-05);
    c = fma(c, u, -1.3888888888888889e-03);
    c = fma(c, u, 4.1666666666666664e-02);
    c = fma(c, u, -0.5);
    c = fma(c, u, 1.0);
    return flip ? -c : c;
}

// what one lane holds, for every lane (t is wave-uniform)
__device__ __forceinline__ double bcast(double v, int t)
{
    const u64 b = __builtin_bit_cast(u64, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, t);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), t);
    return __builtin_bit_cast(double, ((u64)hi << 32) | lo);
}

// the wave's lexicographic minimum of (d, c), in every lane
__device__ __forceinline__ void wave_min(double &d, int &c)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o);
        const int oc = __shfl_xor(c, o);
        if (od < d || (od == d && oc < c)) { d = od; c = oc; }
    }
}

// LDS written by some lanes of the wave is read by others: the wave's LDS operations complete in order, the compiler must
// not move them across this point
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// position of the k-th (from 0) set bit of m; k < popcount(m)
__device__ __forceinline__ int select64(u64 m, int k)
{
    int pos = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int c = __popcll(m & (((1ull << s) - 1ull) << pos));
        if (k >= c) { k -= c; pos += s; }
    }
    return pos;
}

// One wave's slice of LDS: sensed and occupied bit sets (64 cells per word), the prefix popcounts of the list being emitted,
// the nearby-agent masks (64 agents per word), one pass's nearby positions.  The only things sized by the handle.
struct WaveLds {
    int w64, nwa, nbcap;
    __host__ __device__ WaveLds(int ng_max, int n_a)
        : w64((ng_max + 63) >> 6), nwa((n_a + 63) >> 6), nbcap(((n_a + 63) & ~63) < kNbCap ? ((n_a + 63) & ~63) : kNbCap) {}
    __host__ __device__ int off_obits() const { return w64 * 8; }
    __host__ __device__ int off_nbm() const { return w64 * 16; }
    __host__ __device__ int off_nb() const { return off_nbm() + nwa * 8; }
    __host__ __device__ int off_pref() const { return off_nb() + nbcap * 16; }
    __host__ __device__ int bytes() const { return (off_pref() + (w64 + 1) * 4 + 15) & ~15; }
};

// ---- k_large_move: the dynamics of one agent, ENV:515-518,638-652.  act_mode as k_env's: bit 0 doubles, bit 1 the reference's
// (2, n_a) component-major host layout with the envs side by side, else agent-major pairs [E][N][2].  pair_bytes: size of one
// (x, y) pair of the handle's obs dtype; a_prior (may be NULL) receives the prior the previous pass left in prior_next.
__global__ void __launch_bounds__(256)
k_large_move(const KP P, const void *__restrict__ action, const int act_mode, void *__restrict__ a_prior, const int pair_bytes)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n_a = P.n_a;
    if (t >= (long long)P.n_env * n_a) return;
    const int e = (int)(t / n_a), i = (int)(t - (long long)e * n_a);
    const size_t sbase = (size_t)e * 2 * n_a;
    const double px = P.p[sbase + i], py = P.p[sbase + n_a + i];
    const double vx = P.dp[sbase + i], vy = P.dp[sbase + n_a + i];
    const double2 sf = P.sf_next[t];
    double ax, ay;
    if (act_mode & 2) {
        const size_t a0 = (size_t)t, a1 = a0 + (size_t)P.n_env * n_a;
        if (act_mode & 1) { ax = ((const double *)action)[a0]; ay = ((const double *)action)[a1]; }
        else { ax = (double)((const float *)action)[a0]; ay = (double)((const float *)action)[a1]; }
    }
    else if (act_mode & 1) { ax = ((const double *)action)[2 * (size_t)t]; ay = ((const double *)action)[2 * (size_t)t + 1]; }
    else { const float2 af = reinterpret_cast<const float2 *>(action)[t]; ax = (double)af.x; ay = (double)af.y; }
    if (a_prior != nullptr) {
        if (pair_bytes == 16) reinterpret_cast<double2 *>(a_prior)[t] = reinterpret_cast<const double2 *>(P.prior_next)[t];
        else if (pair_bytes == 8) reinterpret_cast<float2 *>(a_prior)[t] = reinterpret_cast<const float2 *>(P.prior_next)[t];
        else reinterpret_cast<unsigned *>(a_prior)[t] = reinterpret_cast<const unsigned *>(P.prior_next)[t];
    }
    double Fx = 1 * ax + sf.x, Fy = 1 * ay + sf.y;                          // ENV:638,640
    if (P.boundary) {                                                       // CPP:817-855, ENV:515-518
        const double d0 = px - P.size_a - P.bx0;
        const double d1 = P.by1 - (py + P.size_a);
        const double d2 = P.bx2 - (px + P.size_a);
        const double d3 = py - P.size_a - P.by3;
        const double a0 = d0 < 0 ? fabs(d0) : 0.0, a1 = d1 < 0 ? fabs(d1) : 0.0;
        const double a2 = d2 < 0 ? fabs(d2) : 0.0, a3 = d3 < 0 ? fabs(d3) : 0.0;
        const double sx_ = (a0 - a2) * P.k_wall, sy_ = (a3 - a1) * P.k_wall;
        const double v0 = d0 < 0 ? vx : 0.0, v2 = d2 < 0 ? vx : 0.0;
        const double v3 = d3 < 0 ? vy : 0.0, v1 = d1 < 0 ? vy : 0.0;
        const double gx = (-v0 - v2) * P.c_wall, gy = (-v3 - v1) * P.c_wall;
        Fx = Fx + sx_ + gx;
        Fy = Fy + sy_ + gy;
    }
    double nvx = vx + (Fx / 1.0) * P.dt, nvy = vy + (Fy / 1.0) * P.dt;      // ENV:643-647
    nvx = nvx < -P.vel_max ? -P.vel_max : (nvx > P.vel_max ? P.vel_max : nvx);
    nvy = nvy < -P.vel_max ? -P.vel_max : (nvy > P.vel_max ? P.vel_max : nvy);
    double npx = px + nvx * P.dt, npy = py + nvy * P.dt;                    // ENV:650
    if (P.periodic) {                                                       // ENV:773-776
        if (npx < P.bx0) npx += 2 * P.w_half;
        if (npx > P.bx2) npx -= 2 * P.w_half;
        if (npy < P.by3) npy += 2 * P.h_half;
        if (npy > P.by1) npy -= 2 * P.h_half;
    }
    P.p[sbase + i] = npx; P.p[sbase + n_a + i] = npy;
    P.dp[sbase + i] = nvx; P.dp[sbase + n_a + i] = nvy;
}

// ---- k_large_observe: the observation pass of one agent per wavefront.  Phases, none with a workgroup barrier:
//   1 pair     lanes over the other agents: candidate bits (per lane), nearby masks (LDS), the contact spring of the next step
//   2 nearest  topo rounds of a wave-wide minimum over the candidates' (norm, index)
//   3 scan     lanes over the cells: sensed words (LDS), first-minimum nearest cell, in-shape flag
//   4 filter   in shape only: lanes over the cells of each non-empty sensed word, nearby agents broadcast from LDS
//   5 lists    lane = slot: rank from the reference's round(i * step), rank -> cell through the prefix popcounts; obs cell pairs,
//              exported lists, the reward's psi terms summed in slot order
//   6 outputs  reward, done, obs head, prior (and the 'llm' twin), exported neighbour list / nearest cell / in-shape flag
template <typename OT>
__global__ void __launch_bounds__(64 * kWaves)
k_large_observe(const KP P, OT *__restrict__ obs, float *__restrict__ reward, uint8_t *__restrict__ done)
{
    typedef typename Pair<OT>::type OT2;
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n_a = P.n_a;
    const long long a = (long long)blockIdx.x * kWaves + wv;
    if (a >= (long long)P.n_env * n_a) return;                              // the whole wave; no barrier follows
    const int e = (int)(a / n_a), i = (int)(a - (long long)e * n_a);

    const WaveLds L(P.ng_max, n_a);
    unsigned char *mine = smem + (size_t)wv * L.bytes();
    u64 *sbits = reinterpret_cast<u64 *>(mine);
    u64 *obits = reinterpret_cast<u64 *>(mine + L.off_obits());
    u64 *nbm = reinterpret_cast<u64 *>(mine + L.off_nbm());
    double2 *nb = reinterpret_cast<double2 *>(mine + L.off_nb());
    int *pref = reinterpret_cast<int *>(mine + L.off_pref());

    const double *__restrict__ pe = P.p + (size_t)e * 2 * n_a;
    const double *__restrict__ ve = P.dp + (size_t)e * 2 * n_a;
    const double px = pe[i], py = pe[n_a + i], vx = ve[i], vy = ve[n_a + i];

    // ---- 1 pair pass.  Candidates: wrapped norm < d_sen, self removed by id (CPP:628-698).  Nearby: UN-wrapped
    // norm < d_sen + r_avoid/2, self included (CPP:155-161).  Contact: un-wrapped centre distance < 2 size_a (ENV:442-457);
    // the spring (CPP:735-815) is summed over the colliding agents in ascending index from +0.0.  An entry (i, k) is
    // collide * d_edge * k_ball * (-(delta / d_center)), delta = p_k - p_i wrapped when periodic; the reference evaluates a
    // pair from the side of the higher index and negates it for the other, which gives the same bits: the subtraction, the
    // wrap and the product are odd in delta.  Its numpy wrap of d_center touches agent 0's row only, which no pair reads.
    unsigned candm = 0;                                                      // bit q: agent 64 q + lane is a candidate
    int n_nb = 0;
    double sfx = 0.0, sfy = 0.0;
    for (int q = 0; q < L.nwa; ++q) {
        const int j = q * 64 + lane;
        const bool in = j < n_a;
        const double xj = in ? pe[j] : 0.0, yj = in ? pe[n_a + j] : 0.0;
        const double dx = xj - px, dy = yj - py;
        const double d2u = dx * dx + dy * dy;
        double rx = dx, ry = dy;
        if (P.periodic) wrap_rel(rx, ry, P.w_half, P.h_half);
        const double d2w = rx * rx + ry * ry;
        if (in && j != i && d2w < P.c_sen) candm |= 1u << q;
        const u64 nm = __ballot(in && d2u < P.c_near);
        if (lane == 0) nbm[q] = nm;
        n_nb += __popcll(nm);
        u64 hm = __ballot(in && j != i && d2u < P.c_ball);
        while (hm) {
            const int k = q * 64 + __ffsll(hm) - 1;
            hm &= hm - 1;
            const double kx = pe[k] - px, ky = pe[n_a + k] - py;
            const double dc = sqrt(kx * kx + ky * ky);
            const double de = fabs(dc - P.size2);
            double wx = kx, wy = ky;
            if (P.periodic) wrap_rel(wx, wy, P.w_half, P.h_half);
            const double ux = wx / dc, uy = wy / dc;
            sfx += 1.0 * de * P.k_ball * (-ux);
            sfy += 1.0 * de * P.k_ball * (-uy);
        }
    }
    if (lane == 0) P.sf_next[a] = make_double2(sfx, sfy);

    // ---- 2 the topo nearest candidates by (norm, index): the norm is the rounded square root, so two squared distances that
    // round to one norm tie and the lower index goes first (CPP:636-641; DESIGN.md deviation 1)
    int nj[kTopoMax];
    bool collision = false;
#pragma unroll
    for (int k = 0; k < kTopoMax; ++k) {
        nj[k] = -1;
        if (k < P.topo) {
            double bd = INFINITY; int bj = INT_MAX;
            unsigned m = candm;
            while (m) {
                const int q = __ffs(m) - 1;
                m &= m - 1;
                const int j = q * 64 + lane;
                double rx = pe[j] - px, ry = pe[n_a + j] - py;
                if (P.periodic) wrap_rel(rx, ry, P.w_half, P.h_half);
                const double d = sqrt(rx * rx + ry * ry);
                if (d < bd) { bd = d; bj = j; }                              // ascending j: the first of equal norms stays
            }
            wave_min(bd, bj);
            if (bj != INT_MAX) {
                nj[k] = bj;
                if ((bj & 63) == lane) candm &= ~(1u << (bj >> 6));
                collision = collision || P.r_avoid > bd;                    // CPP:459-491, on the new list
            }
        }
    }

    // ---- 3 cell scan, _get_target_grid_state CPP:858-908: sensed bits in ascending cell order, first minimum (compared as
    // squared distances: DESIGN.md deviation 2)
    const int ng = P.n_g[e];
    const int W = (ng + 63) >> 6;
    const double2 *__restrict__ gc = P.cells_xy + (size_t)e * P.ng_max;
    double best = INFINITY; int bc = INT_MAX; int n_s = 0;
    for (int w = 0; w < W; ++w) {
        const int c = w * 64 + lane;
        const bool in = c < ng;
        const double2 g = gc[in ? c : 0];
        const double ex = g.x - px, ey = g.y - py;
        const double d2 = ex * ex + ey * ey;
        if (in && d2 < best) { best = d2; bc = c; }
        const u64 sm = __ballot(in && d2 < P.c_sen);
        if (lane == 0) { sbits[w] = sm; obits[w] = 0; }
        n_s += __popcll(sm);
    }
    wave_min(best, bc);
    if (bc == INT_MAX) bc = 0;
    const bool in_shape = best < P.c_in[e];                                  // CPP:889
    const double2 gbest = gc[bc];
    wave_sync();

    // ---- 4 occupied-cell filter, CPP:144-207, as written: a sensed cell is occupied iff some nearby agent j has
    // !(|c - p_j| > r_avoid/2).  No geometric shortcut.
    int n_o = 0;
    if (in_shape && n_s > 0) {
        for (int lo = 0; lo < n_nb; lo += L.nbcap) {
            int base = 0;
            for (int q = 0; q < L.nwa; ++q) {                                // stage the nearby agents of ranks [lo, lo + nbcap)
                const u64 m = nbm[q];
                const int r = base + __popcll(m & ((1ull << lane) - 1ull)) - lo;
                if (((m >> lane) & 1ull) && r >= 0 && r < L.nbcap) { const int j = q * 64 + lane; nb[r] = make_double2(pe[j], pe[n_a + j]); }
                base += __popcll(m);
            }
            wave_sync();
            const int cnt = n_nb - lo < L.nbcap ? n_nb - lo : L.nbcap;
            for (int w = 0; w < W; ++w) {
                const u64 sm = sbits[w];
                if (sm == 0) continue;
                const bool bit = (sm >> lane) & 1ull;
                const double2 g = gc[bit ? w * 64 + lane : 0];
                bool occ = false;
                for (int t = 0; t < cnt; ++t) {
                    const double2 b = nb[t];
                    const double gx = g.x - b.x, gy = g.y - b.y;
                    occ = occ || (gx * gx + gy * gy < P.c_occ);
                }
                const u64 om = __ballot(bit && occ);
                if (lane == 0 && om != 0) obits[w] |= om;
            }
            wave_sync();
        }
        for (int w = 0; w < W; ++w) n_o += __popcll(obits[w]);
    }
    const int n_k = n_s - n_o;

    // exclusive prefix popcounts of the kept (occ == false) or occupied words -> pref[0 .. W)
    auto word = [&](int w, bool occ) -> u64 { return occ ? obits[w] : (sbits[w] & ~obits[w]); };
    auto build_prefix = [&](bool occ) {
        const int per = (W + 63) >> 6;
        int loc = 0;
        for (int t = 0; t < per; ++t) { const int w = lane * per + t; if (w < W) loc += __popcll(word(w, occ)); }
        int inc = loc;
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (lane >= o) inc += v; }
        int run = inc - loc;
        for (int t = 0; t < per; ++t) { const int w = lane * per + t; if (w < W) { pref[w] = run; run += __popcll(word(w, occ)); } }
        wave_sync();
    };
    // the cell of rank r (< the list's count) in ascending cell order
    auto cell_of_rank = [&](int r, bool occ) -> int {
        int lo = 0, hi = W - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pref[mid] <= r) lo = mid; else hi = mid - 1; }
        return lo * 64 + select64(word(lo, occ), r - pref[lo]);
    };

    // ---- 5 the sensed list, its cap (CPP:236-271: dst[i] = src[round(i * step)], std::round; the expert's export pass rounds
    // ties to even as numpy does), the obs cell pairs with zeros behind them (CPP:274-306), the reward's sums (CPP:494-551)
    const int G = P.g_max;
    const int HP = 2 * (P.with_self + P.topo) + 2;                           // head pairs
    OT2 *row = obs != nullptr ? reinterpret_cast<OT2 *>(obs) + (size_t)a * (P.obs_dim >> 1) : nullptr;
    const int n_out = n_k < G ? n_k : G;
    const bool sub = n_k > G;
    const double step = sub ? (double)(n_k - 1) / (G - 1) : 0.0;
    double num0 = 0.0, num1 = 0.0, den = 0.0;
    build_prefix(false);
    for (int base = 0; base < G; base += 64) {
        const int s = base + lane;
        int c = -1;
        double x = 0.0, y = 0.0;
        if (s < n_out) {
            const int r = sub ? (int)(P.cap_even ? rint(s * step) : round(s * step)) : s;
            c = cell_of_rank(r, false);
            const double2 g = gc[c];
            x = g.x - px; y = g.y - py;
        }
        if (s < G) {
            if (row != nullptr) { OT2 o; o.x = to_out<OT>(x); o.y = to_out<OT>(y); store_nt(row + HP + s, o); }
            if (P.export_idx) P.exp_sensed[(size_t)a * G + s] = c;
        }
        if (in_shape && base < n_out) {
            double t0 = 0.0, t1 = 0.0, t2 = 0.0;
            if (s < n_out) {
                const double z = sqrt(x * x + y * y);
                const double psi = z < P.d_sen ? (1.0 / 2.0) * (1.0 + cospi01(z / P.d_sen)) : 0.0;      // _rho_cos_dec(z, 0, d_sen)
                t0 = psi * x; t1 = psi * y; t2 = psi;
            }
            const int m = n_out - base < 64 ? n_out - base : 64;
            for (int t = 0; t < m; ++t) { num0 += bcast(t0, t); num1 += bcast(t1, t); den += bcast(t2, t); }
        }
    }
    bool uniform = false;
    if (in_shape && n_out > 0) {
        if (den == 0) den = 1E-8;
        const double v0 = 1.0 * num0 / den, v1 = 1.0 * num1 / den;
        uniform = sqrt(v0 * v0 + v1 * v1) < 0.05;
    }
    // the occupied list with its own cap, CPP:217-233 (always std::round)
    if (P.export_idx) {
        const int O = P.occ_max;
        const int o_out = n_o < O ? n_o : O;
        const bool osub = n_o > O;
        const double ostep = osub ? (double)(n_o - 1) / (O - 1) : 0.0;
        wave_sync();
        build_prefix(true);
        for (int base = 0; base < O; base += 64) {
            const int s = base + lane;
            int c = -1;
            if (s < o_out) c = cell_of_rank(osub ? (int)round(s * ostep) : s, true);
            if (s < O) P.exp_occ[(size_t)a * O + s] = c;
        }
    }

    // ---- 6 outputs
    if (lane == 0) {
        if (reward != nullptr) __builtin_nontemporal_store((in_shape && !collision && uniform) ? 1.0f : 0.0f, &reward[a]);   // CPP:554-556
        if (done != nullptr) __builtin_nontemporal_store((uint8_t)0, &done[a]);                                            // ENV:480-482
        if (P.export_small) {
#pragma unroll
            for (int k = 0; k < kTopoMax; ++k) if (k < P.topo) P.nei[(size_t)a * P.topo + k] = nj[k];
            P.near_cell[a] = bc;
            P.in_flag[a] = in_shape ? 1 : 0;
        }
    }
    // the head of the row, CPP:102-137: [own state], topo neighbour blocks {rel x, rel y, rel vx, rel vy} (zeros without a
    // neighbour; the relative position wrapped when periodic), the target block.  Lane = value.
    const int NB = P.with_self + P.topo + 1;
    if (row != nullptr && lane < 4 * NB) {
        const int blk = lane >> 2, comp = lane & 3;
        const double own = comp == 0 ? px : comp == 1 ? py : comp == 2 ? vx : vy;
        double val;
        if (P.with_self && blk == 0) val = own;
        else if (blk == NB - 1) {
            if (in_shape) val = own - own;                                   // the target is the agent itself, CPP:889-897
            else val = (comp == 0 ? gbest.x : comp == 1 ? gbest.y : 0.0) - own;
        } else {
            const int k = blk - P.with_self;
            int j = -1;
#pragma unroll
            for (int q = 0; q < kTopoMax; ++q) j = q == k ? nj[q] : j;
            val = 0.0;
            if (j >= 0) {
                const double mj = comp == 0 ? pe[j] : comp == 1 ? pe[n_a + j] : comp == 2 ? ve[j] : ve[n_a + j];
                val = mj - own;
                if (P.periodic && comp < 2) {
                    const double hw = comp == 0 ? P.w_half : P.h_half;
                    if (val < -hw) val += 2 * hw; else if (val > hw) val -= 2 * hw;
                }
            }
        }
        __builtin_nontemporal_store(to_out<OT>(val), reinterpret_cast<OT *>(row) + lane);
    }
    // the prior policy of the NEXT step, calculateActionPrior / robotPolicy CPP:1061-1196, on this state and this neighbour
    // list (ENV:605-624 feeds it exactly these), and its Python twin with the other repulsion gain (ENV:892-940)
    if (P.with_prior) {
        double qx = 0.0, qy = 0.0;
        double tx = px - px, ty = py - py;
        if (!in_shape) { tx = gbest.x - px; ty = gbest.y - py; }
        const double dt_ = sqrt(tx * tx + ty * ty);
        if (dt_ > 0) { qx += P.pk_att * tx / dt_; qy += P.pk_att * ty / dt_; }
        double lx = qx, ly = qy;
        double avx = 0.0, avy = 0.0; int cnt = 0;
#pragma unroll
        for (int k = 0; k < kTopoMax; ++k) {
            const int j = nj[k];
            if (j < 0) continue;
            const double x = px - pe[j], y = py - pe[n_a + j];
            const double d2n = x * x + y * y;
            if (d2n > 0 && d2n < P.c_avoid) {                                // 0 < d < r_avoid, CPP:1166-1174
                const double d = sqrt(d2n);
                const double ux = x / d, uy = y / d;
                const double factor = P.pk_rep * (P.r_avoid / d - 1.0);
                qx += factor * ux; qy += factor * uy;
                if (P.llm) { const double fl = P.pk_llm * (P.r_avoid / d - 1.0); lx += fl * ux; ly += fl * uy; }
            }
            avx += ve[j]; avy += ve[n_a + j]; ++cnt;
        }
        if (cnt > 0) {
            avx /= cnt; avy /= cnt;
            const double sxv = P.pk_ali * (avx - vx), syv = P.pk_ali * (avy - vy);
            qx += sxv; qy += syv; lx += sxv; ly += syv;
        }
        if (lane == 0) {
            OT2 o; o.x = to_out<OT>(clamp_ref(qx, -1.0, 1.0)); o.y = to_out<OT>(clamp_ref(qy, -1.0, 1.0));
            reinterpret_cast<OT2 *>(P.prior_next)[a] = o;
            if (P.llm) { double2 u; u.x = clamp_ref(lx, -1.0, 1.0); u.y = clamp_ref(ly, -1.0, 1.0); P.act_next[a] = u; }
        }
    }
}

template <typename OT>
hipError_t launch_observe(hipStream_t st, const KP &kp, int smem, void *obs, float *reward, uint8_t *done)
{
    const long long EN = (long long)kp.n_env * kp.n_a;
    hipLaunchKernelGGL(k_large_observe<OT>, dim3((unsigned)((EN + kWaves - 1) / kWaves)), dim3(64 * kWaves), (size_t)smem, st, kp,
                       static_cast<OT *>(obs), reward, done);
    return hipGetLastError();
}

}  // namespace

namespace swarm_internal {

int large_lds_bytes(int n_cells_max, int n_agents) { return kWaves * WaveLds(n_cells_max, n_agents).bytes(); }

int large_launch(swarm_env *h, const Pass &ps)
{
    KP tmp;
    const KP &kp = launch_kp(h, ps, 0, tmp);
    const long long EN = (long long)kp.n_env * kp.n_a;
    if (ps.do_step) {
        const int pair_bytes = 2 * (int)obs_elem_bytes(h->cfg.obs_dtype);
        hipLaunchKernelGGL(k_large_move, dim3((unsigned)((EN + 255) / 256)), dim3(256), 0, h->stream, kp, ps.action, ps.act_mode,
                           kp.with_prior ? ps.a_prior : nullptr, pair_bytes);
        HIP_TRY(h, hipGetLastError());
    }
    const int smem = large_lds_bytes(kp.ng_max, kp.n_a);
    HIP_LAUNCHED(h, with_obs_type(h->cfg.obs_dtype, [&](auto t) {
        return launch_observe<typename decltype(t)::type>(h->stream, kp, smem, ps.obs, ps.reward, ps.done);
    }));
    return SWARM_OK;
}

}  // namespace swarm_internal
