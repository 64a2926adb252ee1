// The rule-based expert controller (agent_strategy == 'rule', assembly.py:530-601) for the CURRENT state: the one kernel
// behind swarm_rule_action (env_api.hip) and the rule source of swarm_rollout_expert (rollout.hip).  It consumes what the
// index-export observation pass left in HBM (swarm_expert_view): nearest cell / in-shape flag and the capped sensed-cell list
// (the same filter + np.round(i * step) selection as :544-572).
#include <hip/hip_runtime.h>

#include "swarm_internal.h"

namespace {

using swarm_internal::np_sum_stream;
using swarm_internal::np_clip1;

constexpr int kRuleMaxAgents = 256;                                     // swarm_create's n_agents cap

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

template <int W>
void launch_w(const swarm_expert_view &v, double *act64, float *act32, hipStream_t st)
{
    const dim3 grid(v.n_env), block(v.n_agents <= 64 ? 64 : 256);
    if (act32)
        hipLaunchKernelGGL((k_rule<W, true>), grid, block, 0, st, v, act64, reinterpret_cast<float2 *>(act32));
    else
        hipLaunchKernelGGL((k_rule<W, false>), grid, block, 0, st, v, act64, nullptr);
}

}  // namespace

hipError_t swarm_internal_launch_rule(const swarm_expert_view &v, double *act64, float *act32, hipStream_t st)
{
    switch ((v.n_agents + 63) / 64) {
    case 1: launch_w<1>(v, act64, act32, st); break;
    case 2: launch_w<2>(v, act64, act32, st); break;
    case 3: launch_w<3>(v, act64, act32, st); break;
    default: launch_w<4>(v, act64, act32, st); break;
    }
    return hipGetLastError();
}
