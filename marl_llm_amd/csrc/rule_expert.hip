// The rule-based expert controller (agent_strategy == 'rule', assembly.py:530-601) for the CURRENT state: the one kernel
// behind swarm_rule_action (env_api.hip) and the rule source of swarm_rollout_expert (rollout.hip).  It consumes what the
// index-export observation pass left in HBM (swarm_expert_view): nearest cell / in-shape flag and the capped sensed-cell list
// (the same filter + np.round(i * step) selection as :544-572).
#include <hip/hip_runtime.h>

#include "swarm_internal.h"

namespace {

using swarm_internal::np_sum_stream;
using swarm_internal::np_clip1;

constexpr int kRuleMaxAgents = 256;                                     // swarm_create's n_agents cap without large_swarm: k_rule's

// Every agent of one env per workgroup, one thread per agent, fp64 in numpy's operation order (np.sum's pairwise blocks of 8
// included).  np.cos is numpy's vectorised routine, so v_exp agrees to a few ulp, not bit for bit (tests: 1e-12 absolute on
// the clipped action).  The env's p / dp are staged in LDS once; the `|r| < d_sen` neighbour test runs once per pair into a
// per-agent bit mask of W 64-bit words; the interaction sum then visits the set bits in ascending j, the reference's order.
// Writes the fp64 action and, F32 (a template parameter: either instantiation compiles without the other's stores), its f32
// rounding in the same pass.  F32: act64 is the handle's own scratch (16-byte stores); otherwise a caller's array that
// promises 8-byte alignment only.
template <int W, bool F32>
__global__ void __launch_bounds__(256) k_rule(const swarm_expert_view V, double *__restrict__ act64, float2 *__restrict__ act32)
{
    __shared__ double s_p[2 * kRuleMaxAgents], s_v[2 * kRuleMaxAgents];
    const int N = V.n_agents, e = blockIdx.x, G = V.g_max;
    {
        const double *gp = V.p + (size_t)e * 2 * N, *gv = V.dp + (size_t)e * 2 * N;
        for (int k = threadIdx.x; k < 2 * N; k += blockDim.x) { s_p[k] = gp[k]; s_v[k] = gv[k]; }
    }
    __syncthreads();
    const double *px = s_p, *py = s_p + N, *vx = s_v, *vy = s_v + N;
    const double *gx = V.cells + (size_t)e * 2 * V.ng_max, *gy = gx + V.ng_max;
    const double d_sen = V.d_sen, r_avoid = V.r_avoid;
    const double k_1 = 1, k_2 = 15, k_3 = 17;                                  // :532
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const double xi = px[i], yi = py[i], ui = vx[i], wi = vy[i];
        const bool in_shape = V.in_flag[(size_t)e * N + i] != 0;
        double ent_x = 0.0, ent_y = 0.0;                                       // :538-541
        if (!in_shape) {
            const int bc = V.near_cell[(size_t)e * N + i];
            const double rx = gx[bc] - xi, ry = gy[bc] - yi;
            const double nr = sqrt(rx * rx + ry * ry) + 1e-8;
            ent_x = k_1 * (rx / nr) + (0.0 - ui);
            ent_y = k_1 * (ry / nr) + (0.0 - wi);
        }
        const int *sel = V.exp_sensed + ((size_t)e * N + i) * G;               // capped list, -1 padded (:561-572)
        int n = 0;
        while (n < G && sel[n] >= 0) ++n;
        double exp_x = 0.0, exp_y = 0.0;                                       // :574-584
        if (n > 0) {
            auto psi = [&](double rx, double ry) {                             // _rho_cos_dec(z, 0, d_sen) :846-850
                const double z = sqrt(rx * rx + ry * ry);
                return z < d_sen ? 0.5 * (1.0 + cos(M_PI * (z / d_sen - 0) / (1.0 - 0))) : 0.0;
            };
            const double sx = np_sum_stream(n, [&](int q) { const int c = sel[q]; const double rx = gx[c] - xi, ry = gy[c] - yi; return psi(rx, ry) * rx; });
            const double sy = np_sum_stream(n, [&](int q) { const int c = sel[q]; const double rx = gx[c] - xi, ry = gy[c] - yi; return psi(rx, ry) * ry; });
            double den = np_sum_stream(n, [&](int q) { const int c = sel[q]; return psi(gx[c] - xi, gy[c] - yi); });
            if (den == 0) den = 1e-8;
            exp_x = k_2 * sx / den; exp_y = k_2 * sy / den;
        }
        unsigned long long near[W];                                            // :587-598, neighbours j != i with |r| < d_sen
        int n_near = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            unsigned long long m = 0;
            const int jn = min(64, N - 64 * w);
            for (int b = 0; b < jn; ++b) {
                const int j = 64 * w + b;
                const double rx = px[j] - xi, ry = py[j] - yi;
                m |= (unsigned long long)(j != i && sqrt(rx * rx + ry * ry) < d_sen) << b;
            }
            near[w] = m;
            n_near += __popcll(m);
        }
        double int_x = 0.0, int_y = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            for (unsigned long long m = near[w]; m; m &= m - 1) {
                const int j = 64 * w + __ffsll((long long)m) - 1;
                const double rx = px[j] - xi, ry = py[j] - yi;
                const double nr = sqrt(rx * rx + ry * ry);
                if (nr < r_avoid) {
                    const double c = -k_3 * (r_avoid / nr - 1);
                    int_x += c * rx; int_y += c * ry;
                }
                int_x += 5 * (vx[j] - ui) / n_near; int_y += 5 * (vy[j] - wi) / n_near;
            }
        }
        const double ax = (ent_x + exp_x) + int_x, ay = (ent_y + exp_y) + int_y;
        double2 a;
        a.x = np_clip1(ax);                                                    // np.clip :601
        a.y = np_clip1(ay);
        const size_t row = (size_t)e * N + i;
        if constexpr (F32) {
            reinterpret_cast<double2 *>(act64)[row] = a;
            act32[row] = make_float2((float)a.x, (float)a.y);
        } else {
            act64[2 * row] = a.x;
            act64[2 * row + 1] = a.y;
        }
    }
}

// what lane t holds, for every lane (t is wave-uniform)
__device__ __forceinline__ double bcast(double v, int t)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, t);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), t);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// swarm_internal::np_sum_stream for three sums side by side: f(i, v) fills v[0..2] with the i-th term of each.  Every sum sees
// its own terms in np_sum_stream's order -- eight interleaved partial sums, the same combination, the same tail -- so each
// result is the bits np_sum_stream gives for that sum alone; what the three share is evaluated once.
template <class F>
__device__ inline void np_sum_stream3(int n, F f, double (&res)[3])
{
    double v[3];
    if (n < 8) {
        res[0] = res[1] = res[2] = 0.0;
        for (int i = 0; i < n; ++i) { f(i, v); res[0] += v[0]; res[1] += v[1]; res[2] += v[2]; }
        return;
    }
    double r[3][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { f(k, v); r[0][k] = v[0]; r[1][k] = v[1]; r[2][k] = v[2]; }
    const int n8 = n - (n % 8);
    int i;
    for (i = 8; i < n8; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { f(i + k, v); r[0][k] += v[0]; r[1][k] += v[1]; r[2][k] += v[2]; }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) res[s] = ((r[s][0] + r[s][1]) + (r[s][2] + r[s][3])) + ((r[s][4] + r[s][5]) + (r[s][6] + r[s][7]));
    for (; i < n; ++i) { f(i, v); res[0] += v[0]; res[1] += v[1]; res[2] += v[2]; }
}

constexpr int kLargeWords = 16;                                        // 64-bit neighbour words of one agent: 16 * 64 = 1024 agents

// The same controller for any n_agents up to 64 * kLargeWords (swarm_create's large_swarm cap): the grid is over (env, tile of
// 64 agents), one wave per workgroup, lane = agent, so 64 envs of 1024 agents are 1024 workgroups and not 64.  No LDS: the pair
// test takes 64 agents' positions in one coalesced load, lane b holding agent 64 w + b, and hands them round by readlane.  The neighbour words live in registers: the word loops run
// over the first ceil(N / 64) words only and reach near[] through unrolled selects, so every index is a constant.  Arithmetic, operation order and output forms
// are k_rule's, statement for statement (k_rule keeps its own text: its device code is held identical across changes), except
// that the three list sums run side by side (np_sum_stream3: psi and its cos once per cell, not three times; each sum keeps
// its own order) and that the neighbour test compares the squared distance with c_sen = cut_lt(d_sen), the project's exact
// equivalent of sqrt(d2) < d_sen; so on the same lists the two kernels write the same bits.
template <bool F32>
__global__ void __launch_bounds__(64) k_rule_large(const swarm_expert_view V, const double c_sen, double *__restrict__ act64,
                                                   float2 *__restrict__ act32)
{
    const int N = V.n_agents, G = V.g_max;
    const int tiles = (N + 63) >> 6;
    const int e = blockIdx.x / tiles, lane = threadIdx.x, i_own = (blockIdx.x % tiles) * 64 + lane;
    const int i = min(i_own, N - 1);                                           // lanes past the last agent repeat it and store nothing:
                                                                               // the whole wave reaches the readlanes of the pair test
    const double *px = V.p + (size_t)e * 2 * N, *py = px + N, *vx = V.dp + (size_t)e * 2 * N, *vy = vx + N;
    const double *gx = V.cells + (size_t)e * 2 * V.ng_max, *gy = gx + V.ng_max;
    const double d_sen = V.d_sen, r_avoid = V.r_avoid;
    const double k_1 = 1, k_2 = 15, k_3 = 17;                                  // :532
    const double xi = px[i], yi = py[i], ui = vx[i], wi = vy[i];
    const bool in_shape = V.in_flag[(size_t)e * N + i] != 0;
    double ent_x = 0.0, ent_y = 0.0;                                           // :538-541
    if (!in_shape) {
        const int bc = V.near_cell[(size_t)e * N + i];
        const double rx = gx[bc] - xi, ry = gy[bc] - yi;
        const double nr = sqrt(rx * rx + ry * ry) + 1e-8;
        ent_x = k_1 * (rx / nr) + (0.0 - ui);
        ent_y = k_1 * (ry / nr) + (0.0 - wi);
    }
    const int *sel = V.exp_sensed + ((size_t)e * N + i) * G;                   // capped list, -1 padded (:561-572)
    int n = 0;
    while (n < G && sel[n] >= 0) ++n;
    double exp_x = 0.0, exp_y = 0.0;                                           // :574-584
    if (n > 0) {
        auto psi = [&](double rx, double ry) {                                 // _rho_cos_dec(z, 0, d_sen) :846-850
            const double z = sqrt(rx * rx + ry * ry);
            return z < d_sen ? 0.5 * (1.0 + cos(M_PI * (z / d_sen - 0) / (1.0 - 0))) : 0.0;
        };
        double sums[3];                                                        // np.sum(psi * rel, axis=1), np.sum(psi): psi once per cell
        np_sum_stream3(n, [&](int q, double (&v)[3]) {
            const int c = sel[q];
            const double rx = gx[c] - xi, ry = gy[c] - yi, w = psi(rx, ry);
            v[0] = w * rx; v[1] = w * ry; v[2] = w;
        }, sums);
        const double sx = sums[0], sy = sums[1];
        double den = sums[2];
        if (den == 0) den = 1e-8;
        exp_x = k_2 * sx / den; exp_y = k_2 * sy / den;
    }
    unsigned long long near[kLargeWords] = {};                                 // :587-598, neighbours j != i with |r| < d_sen
    int n_near = 0;
    for (int w = 0; w < tiles; ++w) {                                          // (w is wave-uniform)
        unsigned long long m = 0;
        const int jn = min(64, N - 64 * w), jl = min(64 * w + lane, N - 1);
        const double xl = px[jl], yl = py[jl];
        for (int b = 0; b < jn; ++b) {
            const int j = 64 * w + b;
            const double rx = bcast(xl, b) - xi, ry = bcast(yl, b) - yi;
            m |= (unsigned long long)(j != i && rx * rx + ry * ry < c_sen) << b;      // sqrt(d2) < d_sen, without the sqrt
        }
#pragma unroll
        for (int k = 0; k < kLargeWords; ++k) near[k] = k == w ? m : near[k];
        n_near += __popcll(m);
    }
    double int_x = 0.0, int_y = 0.0;
    for (int w = 0; w < tiles; ++w) {
        unsigned long long m = 0;
#pragma unroll
        for (int k = 0; k < kLargeWords; ++k) m = k == w ? near[k] : m;
        for (; m; m &= m - 1) {
            const int j = 64 * w + __ffsll((long long)m) - 1;
            const double rx = px[j] - xi, ry = py[j] - yi;
            const double nr = sqrt(rx * rx + ry * ry);
            if (nr < r_avoid) {
                const double c = -k_3 * (r_avoid / nr - 1);
                int_x += c * rx; int_y += c * ry;
            }
            int_x += 5 * (vx[j] - ui) / n_near; int_y += 5 * (vy[j] - wi) / n_near;
        }
    }
    const double ax = (ent_x + exp_x) + int_x, ay = (ent_y + exp_y) + int_y;
    double2 a;
    a.x = np_clip1(ax);                                                        // np.clip :601
    a.y = np_clip1(ay);
    if (i_own >= N) return;
    const size_t row = (size_t)e * N + i;
    if constexpr (F32) {
        reinterpret_cast<double2 *>(act64)[row] = a;
        act32[row] = make_float2((float)a.x, (float)a.y);
    } else {
        act64[2 * row] = a.x;
        act64[2 * row + 1] = a.y;
    }
}

template <int W>
void launch_w(const swarm_expert_view &v, double *act64, float *act32, hipStream_t st)
{
    const dim3 grid(v.n_env), block(v.n_agents <= 64 ? 64 : 256);
    if (act32)
        hipLaunchKernelGGL((k_rule<W, true>), grid, block, 0, st, v, act64, reinterpret_cast<float2 *>(act32));
    else
        hipLaunchKernelGGL((k_rule<W, false>), grid, block, 0, st, v, act64, nullptr);
}

// (a template, first named behind launch_w in swarm_internal_launch_rule, so that k_rule's instantiations stay the first functions of
// the unit: tools/isa_diff.py then finds k_rule's text unchanged, local label numbers included)
template <bool F32>
void launch_large(const swarm_expert_view &v, double *act64, float *act32, hipStream_t st)
{
    const dim3 grid((unsigned)v.n_env * (unsigned)((v.n_agents + 63) / 64)), block(64);
    const double c_sen = swarm_internal::cut_lt(v.d_sen);                      // |r| < d_sen  <=>  r . r < c_sen (DESIGN "Numerics")
    hipLaunchKernelGGL((k_rule_large<F32>), grid, block, 0, st, v, c_sen, act64, reinterpret_cast<float2 *>(act32));
}

}  // namespace

hipError_t swarm_internal_launch_rule(const swarm_expert_view &v, double *act64, float *act32, hipStream_t st, bool tiled)
{
    if (!tiled && v.n_agents <= kRuleMaxAgents) {
        switch ((v.n_agents + 63) / 64) {
        case 1: launch_w<1>(v, act64, act32, st); break;
        case 2: launch_w<2>(v, act64, act32, st); break;
        case 3: launch_w<3>(v, act64, act32, st); break;
        default: launch_w<4>(v, act64, act32, st); break;
        }
    } else if (act32) {
        launch_large<true>(v, act64, act32, st);
    } else {
        launch_large<false>(v, act64, nullptr, st);
    }
    return hipGetLastError();
}
