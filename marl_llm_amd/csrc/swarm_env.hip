// swarm_env.hip -- MI355X (gfx950 / CDNA4) batched AssemblySwarm environment step: the kernel, its LDS map and its launch.
// Only what determines the step kernel's device code lives here (bench.py and tools/pmc_summary.py identify the kernel by
// this file's hash): the side kernels are in env_kernels.hip, the handle and the C ABI in env_api.hip, the kernel-argument
// struct KP and the handle's declaration in env_types.h.
//
// One fused kernel advances E independent environments by one AssemblySwarmEnv.step():
//   contact / wall forces -> prior policy -> semi-implicit Euler -> neighbour search ->
//   target-cell scan -> occupied-cell filter -> capped sensed list -> reward -> observation rows.
// Reference semantics being reproduced (never copied):
//   ENV = /root/reference/cus_gym/gym/envs/customized_envs/assembly.py
//   CPP = /root/reference/cus_gym/gym/envs/customized_envs/envs_cplus/src/AssemblyEnv.cpp
//
// Mapping: lane = agent.  NPAD (agents per env rounded up to a power of two, 8..256) is a template
// parameter; a 64-wide wavefront holds 64/NPAD whole environments when NPAD < 64, and an environment
// of 128/256 agents takes 2/4 wavefronts.  A workgroup holds WPE copies ("splits") of its agent threads
// that share the env's LDS footprint: sequential per-agent work (forces, prior, ordered neighbour
// insertion, reward decision) runs on one split each, everything else is dealt over all of them.
// Agent positions / velocities live in LDS and are read with wave-uniform addresses (LDS broadcast).
// Target cells: when they form a lattice (the reference's tiled shapes always do) the sensed / covered /
// nearest-cell queries walk lattice ROWS with bit operations on row masks and need no coordinates; the
// exact fp64 coordinates are gathered from an interleaved copy in global memory only where a value or an
// exact tie-break needs them.  Arbitrary cell sets take an fp32 pre-filter scan with exact fp64 fallback.
// The observation block of an environment is streamed out with consecutive lanes writing consecutive
// addresses (the rows of one env are contiguous in HBM).  DESIGN.md section 3 has the phase list.
//
// Numerics: everything that decides an index, a flag, the state or the reward is IEEE double in the
// reference's operation order; this file MUST be compiled with -ffp-contract=off (the reference is
// built for baseline x86-64, no FMA).  Threshold tests of the form sqrt(d2) < t are evaluated as
// d2 < cut(t) with cut(t) = the smallest double whose correctly rounded sqrt is >= t, computed on the
// host; sqrt is monotonic, so the two tests are equivalent bit for bit and the scans need no sqrt.
//
// There is no CPU path in this file.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>

#include "swarm_env.h"
#include "env_types.h"

using namespace swarm_internal;

// One source, several objects (marl_llm_amd/build.py: UNITS).  SWARM_ENV_UNIT chooses what a compile of this file holds:
//   8, 16, 32, 64, 128, 256   a KERNEL unit: the k_env instantiations of that padded agent count, launch_t / launch_n and
//                             the one function the rest of the library calls, swarm_internal::launch_npad<NPAD>
//   0                         the HOST unit: layout_t, the geometries, env_launch, the swarm_debug_* entry points; no kernel
//   (not defined)             everything, as one translation unit -- what an ad-hoc hipcc line gets, and the witness that the
//                             cut changes no kernel (tools/isa_diff.py)
// The kernel's text is in this file alone, whatever the cut.  Geo and LatMap are visible to every unit.
#if !defined(SWARM_ENV_UNIT)
#define SWARM_UNIT_KERNELS 1
#define SWARM_UNIT_HOST 1
#elif SWARM_ENV_UNIT == 0
#define SWARM_UNIT_KERNELS 0
#define SWARM_UNIT_HOST 1
#else
#define SWARM_UNIT_KERNELS 1
#define SWARM_UNIT_HOST 0
#endif

namespace {

typedef unsigned long long u64;

typedef float f2v __attribute__((ext_vector_type(2)));

template <typename T> struct Pair;
template <> struct Pair<float>  { typedef float2 type; };
template <> struct Pair<double> { typedef double2 type; };
typedef __attribute__((ext_vector_type(2))) __bf16 bf2v;
template <> struct Pair<__bf16> { typedef bf2v type; };

// output conversion of an exact fp64 value: one rounding for f64 / f32; bf16 = the f32 value rounded again (RNE), i.e. what a
// consumer gets from `obs_f32.to(bfloat16)`
template <typename OT> __device__ __forceinline__ OT to_out(double v) { return (OT)v; }
// streaming store of one observation pair: the observation block (768 B per agent and step, written once, read by another
// kernel) would otherwise sweep the target cells, lattice rows and agent state of every environment out of the L2 between
// launches; the non-temporal hint keeps those resident for the next step's gathers
typedef double d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_nt(float2 *dst, float2 v) { f2v t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<f2v *>(dst)); }
__device__ __forceinline__ void store_nt(double2 *dst, double2 v) { d2v t = {v.x, v.y}; __builtin_nontemporal_store(t, reinterpret_cast<d2v *>(dst)); }
__device__ __forceinline__ void store_nt(bf2v *dst, bf2v v) { __builtin_nontemporal_store(v, dst); }
template <> __device__ __forceinline__ __bf16 to_out<__bf16>(double v) { return (__bf16)(float)v; }

__device__ __forceinline__ void wrap_rel(double &x, double &y, double wh, double hh)
{   // CPP:700-715
    if (x < -wh) x += 2 * wh; else if (x > wh) x -= 2 * wh;
    if (y < -hh) y += 2 * hh; else if (y > hh) y -= 2 * hh;
}

// gfx950 hazard: a VALU instruction that reads an SGPR (lane mask / scalar source) written by a VALU instruction -- the
// v_cmp that produced the mask -- needs two wait states in between.  The compiler's hazard recogniser inserts them for its
// own instructions but cannot see inside inline asm, so both helpers below carry their own `s_nop 1` (it stalls only this
// wave for two cycles; other waves issue meanwhile).  Without it the asm reads a stale mask whenever the scheduler happens
// to place it right behind the compare.

// old[LANE] = value (wave-uniform value, compile-time lane): one v_writelane_b32 (the lane select must be an
// inline constant: a second SGPR operand would violate the constant-bus limit).
template <int LANE>
__device__ __forceinline__ int writelane_c(int value, int old)
{
    asm("s_nop 1\n\tv_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(value), "n"(LANE));
    return old;
}

// (acc << 1) | bit, the bit coming per lane from a 64-bit lane mask (a compare result): ONE v_addc_co_u32 with
// the mask as carry-in.
__device__ __forceinline__ unsigned shl1_or_mask(unsigned acc, unsigned long long mask)
{
    unsigned long long carry_out;
    asm("s_nop 1\n\tv_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(acc), "=s"(carry_out) : "v"(acc), "s"(mask));
    return acc;
}

// The pair pass's five threshold tests of one (i, j) pair in ONE asm block: all compares first, then all add-with-carry
// accumulations (acc = 2 acc + test).  The compare that feeds an accumulation is at least four instructions ahead of it, so
// the VALU-writes-SGPR -> VALU-reads-it hazard (two wait states) is covered by the block's own instructions: no s_nop at all
// (shl1_or_mask pays one per test).  d2u: un-wrapped squared distance (nearby / exception band / contact), d2: wrapped
// (candidates, close candidates).
__device__ __forceinline__ void pair_tests5(double d2u, double d2, double c_nb, double c_hi, double c_ht, double c_cd, double c_c1,
                                            unsigned &nb, unsigned &hi, unsigned &ht, unsigned &cd, unsigned &c1)
{
    unsigned long long m0, m1, m2, m3, m4;
    asm("v_cmp_lt_f64_e64 %5, %10, %12\n\t"
        "v_cmp_lt_f64_e64 %6, %10, %13\n\t"
        "v_cmp_lt_f64_e64 %7, %10, %14\n\t"
        "v_cmp_lt_f64_e64 %8, %11, %15\n\t"
        "v_cmp_lt_f64_e64 %9, %11, %16\n\t"
        "v_addc_co_u32_e64 %0, %5, %0, %0, %5\n\t"
        "v_addc_co_u32_e64 %1, %6, %1, %1, %6\n\t"
        "v_addc_co_u32_e64 %2, %7, %2, %2, %7\n\t"
        "v_addc_co_u32_e64 %3, %8, %3, %3, %8\n\t"
        "v_addc_co_u32_e64 %4, %9, %4, %4, %9"
        : "+v"(nb), "+v"(hi), "+v"(ht), "+v"(cd), "+v"(c1), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4)
        : "v"(d2u), "v"(d2), "s"(c_nb), "s"(c_hi), "s"(c_ht), "s"(c_cd), "s"(c_c1));
}

// The same with the sixth test of the N > 128 instantiations (the wider pre-selection ring) in the block: the test costs its
// compare and its accumulation, no wait state.
__device__ __forceinline__ void pair_tests6(double d2u, double d2, double c_nb, double c_hi, double c_ht, double c_cd, double c_c1, double c_c2,
                                            unsigned &nb, unsigned &hi, unsigned &ht, unsigned &cd, unsigned &c1, unsigned &c2)
{
    unsigned long long m0, m1, m2, m3, m4, m5;
    asm("v_cmp_lt_f64_e64 %6, %12, %14\n\t"
        "v_cmp_lt_f64_e64 %7, %12, %15\n\t"
        "v_cmp_lt_f64_e64 %8, %12, %16\n\t"
        "v_cmp_lt_f64_e64 %9, %13, %17\n\t"
        "v_cmp_lt_f64_e64 %10, %13, %18\n\t"
        "v_cmp_lt_f64_e64 %11, %13, %19\n\t"
        "v_addc_co_u32_e64 %0, %6, %0, %0, %6\n\t"
        "v_addc_co_u32_e64 %1, %7, %1, %1, %7\n\t"
        "v_addc_co_u32_e64 %2, %8, %2, %2, %8\n\t"
        "v_addc_co_u32_e64 %3, %9, %3, %3, %9\n\t"
        "v_addc_co_u32_e64 %4, %10, %4, %4, %10\n\t"
        "v_addc_co_u32_e64 %5, %11, %5, %5, %11"
        : "+v"(nb), "+v"(hi), "+v"(ht), "+v"(cd), "+v"(c1), "+v"(c2), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5)
        : "v"(d2u), "v"(d2), "s"(c_nb), "s"(c_hi), "s"(c_ht), "s"(c_cd), "s"(c_c1), "s"(c_c2));
}

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N-1>{})
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    static_for_impl(static_cast<F &&>(f), std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ double clamp_ref(double v, double lo, double hi)
{   // CPP:11-14  std::max(lo, std::min(v, hi))
    double m = (hi < v) ? hi : v;
    return (lo < m) ? m : lo;
}

// The ablation hooks (tools/ablate.py): run phase k EXTRA more times; leave the kernel after segment k.  DIAG is a constexpr
// of the instantiation (k_env): the lattice kernels of 64 agents carry the hooks only in a library built with -DSWARM_DIAG
// -- there REPS(k) is the constant 1 and EXIT_AT(k) is empty, and KP::dbg_phase / dbg_extra are never read -- every other
// kernel always does.
#ifdef SWARM_DIAG
constexpr bool kDiagBuild = true;
#else
constexpr bool kDiagBuild = false;
#endif
#define REPS(k) (DIAG ? ((P.dbg_phase == (k)) ? P.dbg_extra + 1 : 1) : 1)
#define FENCE() asm volatile("" ::: "memory")
// diagnostics only (tools/ablate.py --cumulative): leave the kernel after segment k (debug phase 15, extra = k); outputs
// are then incomplete, so only timing / counter runs use it
#define EXIT_AT(k) do { if constexpr (DIAG) { if (P.dbg_phase == 15 && P.dbg_extra == (k)) return; } } while (0)

#ifdef SWARM_STAMPS
// written straight to global memory by lane 0 of every wave (no registers held across the kernel)
#define STAMP(k) do { __builtin_amdgcn_sched_barrier(0); if (P.stamps != nullptr && (threadIdx.x & 63) == 0) P.stamps[((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 24 + (k)] = clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define STAMP(k) do { } while (0)
#endif

// Workgroup geometry.  AG "agent threads" hold the agents of the workgroup's environment(s) (lane = agent);
// the workgroup has WPE = 4 copies ("splits") of them (256 agents: 1024 threads).  Splits "A" and "B" own the
// per-agent sequential work (forces / integration / reward decision; prior / ordered neighbour insertion); rows,
// words, slots and rank ranges of the other phases are dealt over all splits.  One environment's LDS footprint is
// thereby shared by four times more wavefronts, which is what buys the occupancy that hides the LDS / fp64 latencies.
// HALF (N < 64, lattice launches, small grids): only half of the 64 agent threads hold agents -- half as many environments
// per workgroup, twice as many workgroups -- and the list phase gives every agent EIGHT lanes instead of four.  A batch that
// fills a fraction of the chip (32 agents x 1024 envs: 512 workgroups on 256 CUs) is bound by the length of one workgroup's
// serial chain, not by throughput: shorter chains on more workgroups.
template <int NPAD, bool HALF = false> struct Geo {
    static_assert(!HALF || NPAD < 64, "the half-occupied geometry is for N < 64");
    static constexpr int NPAD_ = NPAD; static constexpr bool HALF_ = HALF;
    // lattice launches address LDS through LatMap's compile-time offsets.  Not the full-occupancy geometries of N < 64 (several
    // environments per wavefront): measured at 32 x 8192 the constants LOSE 0.8 % there (97.25 -> 98.01 us, three alternating
    // rounds, spread 0.5; fewer VGPRs and less code, the same occupancy -- the schedule that comes out is the slower one).  N = 8 and 16 run the
    // same code shape and were not measured with the constants, so all three keep the run-time offsets and the code they had.
    static constexpr bool CT_MAP = NPAD >= 64 || HALF;
    static constexpr int AG = NPAD < 64 ? 64 : NPAD;
    static constexpr int EPB = NPAD < 64 ? (64 / NPAD) / (HALF ? 2 : 1) : 1;
    static constexpr int ACTW = NPAD < 64 ? EPB * NPAD : 64;     // agent threads of a 64-group that hold agents
    static constexpr int LPA = HALF ? 8 : 4;                     // lanes per agent in the list phase
    static constexpr int AGW = 64 / LPA;                         // agents per wave there (= ACTW / 4)
    static constexpr int NW = AG / 64;
    static constexpr int WPE = 4;
    static constexpr int T = AG * WPE;
#ifndef SWARM_WPS
#define SWARM_WPS 7
#endif
#ifndef SWARM_WPS_SMALL
#define SWARM_WPS_SMALL 6
#endif
    // waves per SIMD the register allocation aims for.  N = 64, lattice kernels: SEVEN 4-wave workgroups per CU (<= 72 VGPRs --
    // the allocator needs 65 -- and 22,976 B of LDS each: 18 of the CU's 128 allocation granules of 1280 B; the kernel loses
    // 7 % from six to five workgroups per CU and gains 4 % from six to seven).  N < 64 (several environments per wavefront:
    // their lattice tables make it 19 - 21 granules): six (76 - 78 VGPRs, no scratch; 32 x 8192: 103.6 -> 97.0 us against
    // five).  N = 128 (512 threads, ~47 KB of LDS): three workgroups per CU instead of two (80 VGPRs, 24 B of scratch;
    // 128 x 4096: 218 -> 185 us).  The generic-scan kernels: six / five.  N = 256: one 16-wave workgroup per CU.
#ifndef SWARM_WPS_128
#define SWARM_WPS_128 6
#endif
    static constexpr int WPS_LAT = NPAD == 64 ? SWARM_WPS : (NPAD < 64 ? SWARM_WPS_SMALL : (NPAD == 128 ? SWARM_WPS_128 : 1));
    static constexpr int WPS_GEN = NPAD == 64 ? 6 : (NPAD < 64 ? 5 : 1);
};

// LDS map of the lattice (row-space) launches, shared by the kernel and by the host's layout_t: every region but the last
// has a size that depends on the geometry alone, so its offset is a compile-time constant (folded into the ds_*
// instructions' immediate offsets: no scalar base, no vector add per region).  The sensed lists `sidx` come LAST: their size
// depends on g_max (KP::g_stride); the export-only `orow` follows them at a run-time offset (KP::off_orow).  Regions that
// share bytes, and why they may:
//   pm   over sidx   the partial pair masks are consumed two barriers before the first list slot is written
//   perm over part_d written two barriers after the walking splits' distances were consumed
//   tgt  over part_d behind perm's bytes: the nearest cell relative to its agent, {x, y} in fp64 (N = 64: the kernels whose
//                    heads and prior read it, TGT_LDS).  Written behind the barrier that ends (K) -- until then another split
//                    may still be merging the distances -- and read behind the one that ends (S)
//   prk  over part_c the partial ranks: the nearest-cell candidates are consumed by the merge, a barrier earlier
//   the exact reward's scratch (N > 64) over srow
template <int NPAD, bool HALF> struct LatMap {
    typedef Geo<NPAD, HALF> G_;
    static constexpr int AG = G_::AG, EPB = G_::EPB, NW = G_::NW, WPE = G_::WPE, T = G_::T;
    static constexpr int NRC = 16;                                        // window rows stored per agent (lat_nrs <= 15)
    static constexpr int al(int bytes) { return (bytes + 15) & ~15; }
    static constexpr int mx(int a, int b) { return a > b ? a : b; }
    static constexpr int sp_bytes = 4 * AG * 8;
    static constexpr int hdr_bytes = AG * 16;
    static constexpr int rew_scratch_bytes = NW * 1536;
    static constexpr int srow_bytes = mx((NRC - 1) * AG * 4, rew_scratch_bytes);
    static constexpr int pcr_bytes = AG * NRC;
    static constexpr int partc_bytes = WPE * AG * 2;
    static constexpr int partd_bytes = (WPE - 1) * AG * 8;
    static constexpr int lat_bytes = EPB * 64 * (8 + 2);
    static constexpr int cov_bytes = EPB * 64 * 8;
    static constexpr int flag_bytes = AG;                                 // one byte per agent thread
    static constexpr int snei_bytes = AG * kNeiStride * 2;
    static constexpr int sncf_bytes = AG * 4;
    static constexpr int snear_bytes = NW > 1 ? NW * AG * 8 : 0;          // (N <= 64: the nearby mask stays in a register)
    static constexpr int orow_bytes = NRC * AG * 4;
    static constexpr int pm_bytes = (NW == 1 ? WPE * 4 : 5) * NW * AG * 8;   // partial pair masks (per-split copies for N <= 64, one accumulator set above)
    static constexpr int sp = 0;
    static constexpr int hdr = sp + al(sp_bytes);
    static constexpr int srow = hdr + al(hdr_bytes);
    static constexpr int pcr = srow + al(srow_bytes);
    static constexpr int partc = pcr + al(pcr_bytes);
    static constexpr int partd = partc + al(partc_bytes);
    static constexpr int lat = partd + al(partd_bytes);
    static constexpr int cov = lat + al(lat_bytes);
    static constexpr int flag = cov + al(cov_bytes);
    static constexpr int snei = flag + al(flag_bytes);
    static constexpr int sncf = snei + al(snei_bytes);
    static constexpr int snear = sncf + al(sncf_bytes);
    static constexpr int sidx = snear + al(snear_bytes);
    static constexpr int perm = partd;
    static constexpr int perm_bytes = T, prk_bytes = WPE * AG * 2;
    static constexpr int tgt = partd + al(perm_bytes);                    // behind perm: the two are live together
    static constexpr int tgt_bytes = AG * 16;
    static constexpr int sidx_bytes(int g_stride) { return al(mx(AG * g_stride * 2, pm_bytes)); }
    static constexpr int total(int g_stride) { return sidx + sidx_bytes(g_stride); }                  // a step launch
    static constexpr int orow_off(int g_stride) { return total(g_stride); }
    static constexpr int total_export(int g_stride) { return orow_off(g_stride) + al(orow_bytes); }   // a launch that exports the lists
    static_assert(perm_bytes <= partd_bytes, "perm must fit the distance array it reuses");
    static_assert(tgt % 16 == 0 && tgt - partd + tgt_bytes <= partd_bytes, "perm and the relative targets must fit the distance array they reuse, side by side");
    static_assert(prk_bytes <= partc_bytes, "the partial ranks must fit the nearest-cell candidates they reuse");
    static_assert(rew_scratch_bytes <= srow_bytes, "the exact reward's scratch must fit the window rows it reuses");
    static_assert(pm_bytes <= sidx_bytes(0), "the pair masks must fit the list region they reuse");
};


// cos(pi * t) for t in [0, 1], absolute error ~2e-16 (Taylor in x = pi*min(t, 1-t) <= pi/2 up to x^22).
// Only the reward's psi weights use it (CPP:1012-1020 calls libm cos(M_PI * z / r)); it is not bit-identical
// to glibc's cos and does not need to be: it feeds a sum that is compared with a threshold.
__device__ __forceinline__ double cospi01(double t)
{
    const bool flip = t > 0.5;
    const double r = flip ? 1.0 - t : t;
    const double x = M_PI * r;
    const double u = x * x;
    double c = -8.8967913924505741e-22;                 // -1/22!
    c = fma(c, u, 4.1103176233121648e-19);              // +1/20!
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

// fp32 fast path of the reward weight: psi(u) = 1/2 (1 + cos(pi sqrt(u))), u = (z/d_sen)^2 in [0, 1], as a
// degree-6 minimax polynomial in u (cos(pi sqrt(u)) is entire in u): no sqrt, no range reduction.
// |abs err| < 3e-7 in fp32 Horner form (fit error 5.5e-9).
__device__ __forceinline__ float psi_u_f32(float u)
{
    float c = 7.969553699e-04f;
    c = fmaf(c, u, -1.267949212e-02f);
    c = fmaf(c, u, 1.175149009e-01f);
    c = fmaf(c, u, -6.675792336e-01f);
    c = fmaf(c, u, 2.029347420e+00f);
    c = fmaf(c, u, -2.467400551e+00f);
    c = fmaf(c, u, 1.0f);
    return c;
}

// The same weight as a degree-5 polynomial (Chebyshev-node fit; |abs err| < 6.5e-7 in fp32 Horner form): one fused multiply-add
// less per kept cell in the lattice path's list walk; the reward's guard band there allows 1.2e-6 for it (set_lattice_mode).
__device__ __forceinline__ float psi5_u_f32(float u)
{
    float c = -1.028585434e-02f;
    c = fmaf(c, u, 1.148182452e-01f);
    c = fmaf(c, u, -6.661784649e-01f);
    c = fmaf(c, u, 2.029018402e+00f);
    c = fmaf(c, u, -2.467372179e+00f);
    c = fmaf(c, u, 9.999995828e-01f);
    return c;
}

// The list walk of the LIST_LEAN kernels (k_env, part (E)): one lane emits the kept cells of ranks k0 .. k1 - 1 of its agent's
// list into `row` and sums their exploration-reward terms, as the plain loop of k_env does -- the same cells in the same order,
// so the slots and the fp32 sums are that loop's bit for bit -- in fewer instructions per cell:
//  - A lane that has cells left always holds a window row with a kept bit, so a trip is one predicated block: the cell, and
//    behind it ONE test "cells left" that also ends the loop.  Under the cap the slot address is the counter (it steps by one
//    slot and is compared with the range's end address).
//  - The next window row's word and its lattice row mask are read one row ahead of their use: a row change takes them from
//    registers and issues the reads of the row after, so no trip waits on a read it has just issued.  A row that kept no cell
//    is stepped over inside the trip, by a loop of its own off the usual path (dbf takes the same additions of inv_r as in the
//    plain loop).  A lane at its range's end steps one row on for nothing, and the reads ahead may pass the window's last row
//    by two: they stay inside the launch's LDS and their values are never used.
//  - The first cell of the range: the position of the set bit of rank `left` in the row by five popcounts of a low part of the
//    word against `left` itself.
//  - CAP (a wave that holds an agent over the cap G): `take` -- the cell's rank is the next selected one, or the agent is
//    under the cap -- is one predicate for the store, the slot and the next selected rank.
// srp / rmp: the window row / lattice row mask of the range's first cell, left = k0 - (kept cells in front of that row).
template <bool CAP, int AG>
__device__ __forceinline__ void list_walk_lean(const KP &P, const unsigned *srp, const u64 *rmp, const int aca0, const int k0,
                                               const int k1, const int left, const int nk, float dbf, const float inv_r,
                                               const float apr_s, short *row, float &n0, float &n1, float &dn)
{
    const int G = P.g_max;
    const unsigned nm1 = (unsigned)(nk - 1);
    const unsigned wd0 = *srp;
    u64 rm0 = *rmp;
    srp += AG; ++rmp;
    unsigned nw = *srp;                                          // one row ahead
    u64 nm = *rmp;
    unsigned kept = k0 < k1 ? (wd0 & 0x1FFFFu) : 0u;
    {
        int pb = 0;
#pragma unroll
        for (int sh = 16; sh >= 1; sh >>= 1) {
            const int c = __popc(__builtin_amdgcn_ubfe(kept, 0u, (unsigned)(pb + sh)));   // pb + sh <= 31
            pb = c <= left ? pb + sh : pb;
        }
        kept = (kept >> pb) << pb;
    }
    int base = (int)(wd0 >> 17);
    unsigned relm = (unsigned)(rm0 >> aca0);
    float db2 = dbf * dbf;
    auto rank_of = [&](int q) -> int {                               // as in k_env
        if (P.cap_int) {
            const unsigned x = 2u * (unsigned)q * nm1 + (unsigned)(G - 1);
            const unsigned hq_ = __umulhi(x, P.cap_magic);
            return (int)((((x - hq_) >> 1) + hq_) >> P.cap_shift);
        }
        const double v = q * ((double)nm1 / (G - 1));
        return (int)(P.cap_even ? rint(v) : round(v));
    };
    const bool cap = CAP && nk > G;
    int k = k0, slot = k0, nxt = 0;
    if constexpr (CAP) {
        if (cap) {
            if (P.cap_int) slot = k0 > 0 ? (int)((unsigned)((2 * k0 - 1) * (G - 1) + 2 * (int)nm1 - 1) / (2u * nm1)) : 0;
            else {
                slot = 0;
#pragma clang loop vectorize(disable) interleave(disable)
                while (slot < G && rank_of(slot) < k0) ++slot;
            }
            slot = slot < G ? slot : G;
            nxt = slot < G ? rank_of(slot) : 0x7FFFFFFF;
        }
    }
    short *p = row + k0;
    const short *const pend = row + k1;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 n10 = {n1, n0};
    auto more = [&]() -> bool { return CAP ? k < k1 : p < pend; };
    while (__any(more())) {
        if (more()) {                                                // kept != 0 here
            const int c = __builtin_ctz(kept);
            kept &= kept - 1;
            const int cell = base + __popc(relm & ((1u << c) - 1u));
            const float da = fmaf((float)c, inv_r, -apr_s);
            const float u = fmaf(da, da, db2);
            float psi = psi5_u_f32(u);
            if constexpr (CAP) {
                const bool take = !cap || k == nxt;
                if (take) {
                    row[slot] = (short)cell;
                    ++slot;
                    if (cap) nxt = slot < G ? rank_of(slot) : 0x7FFFFFFF;
                }
                psi = take ? psi : 0.0f;
                ++k;
            } else {
                *p = (short)cell;
                asm volatile("" ::: "memory");                       // (the store in front of the address's step: no copy of p)
                ++p;
            }
            // n1 += psi dbf, n0 += psi da: one packed fma (each half an fmaf).  The sums stay in front of the row change:
            // sunk behind it they cost a copy of dbf and db2 per trip
            n10 = __builtin_elementwise_fma(f32x2{psi, psi}, f32x2{dbf, da}, n10); dn += psi;
            asm volatile("" : "+v"(n10), "+v"(dn));
            if (kept == 0) {                                         // (a lane at its range's end steps once more, for nothing)
                kept = nw & 0x1FFFFu; base = (int)(nw >> 17);
                relm = (unsigned)(nm >> aca0);
                dbf += inv_r;
                if (__builtin_expect(kept == 0, 0)) {                // a row that kept no cell: stepped over within the trip
                    while (kept == 0 && more()) {
                        srp += AG; ++rmp;
                        const unsigned wd = *srp;
                        kept = wd & 0x1FFFFu; base = (int)(wd >> 17);
                        relm = (unsigned)(*rmp >> aca0);
                        dbf += inv_r;
                    }
                }
                srp += AG; ++rmp;
                nw = *srp; nm = *rmp;                                // the row after, ahead of its use
                db2 = dbf * dbf;
            }
        }
    }
    n1 = n10.x; n0 = n10.y;
}

// The nearest-cell candidates of the lattice rows b = wr, wr + WS, ... < nrows of one env for the WALK_LEAN kernels (k_env,
// part 3): per row the nearest set column below the split column a_r (`dn`) and from it on (`up`), best and runner-up d2
// in lattice units, and the cell index of the best (0 when the lane is inactive or saw no cell).  MT: the row-mask word.
// What row_cands + the plain loop of k_env compute, in fewer instructions per row:
//  - A side without a set column is not selected to +inf: the raw first-bit instructions answer 0xFFFFFFFF for a zero word,
//    which the saturating adds (up) and the xor (down) keep >= 0xFFFFFFC0, so the column converts to ~4.29e9 and the
//    candidate's d2 is >= 1.8e19 whatever the agent's coordinates within coord_lim (lanes outside it take the exact scan).
//    Every real candidate has the operands and the operations of row_cands, so its d2 is that bit for bit.  A second32
//    at or above kNoCand means that no second candidate was seen.
//  - The loop tracks WHICH candidate leads (its trip, row in the trip and side), not its cell index: the winner's
//    rowstart + popcount is worked out once behind the loop.
//  - Four rows a trip: one address, the rows of the trip in the reads' offset fields; the candidate number 0..7 is an inline
//    constant of the select, the trip is noted once, behind its rows.  The last trip holds one to three rows: the rows past
//    the lattice's last are empty words there, candidates at the sentinel distance.
//  - Inactive lanes walk along (their coordinates are whatever the state buffer holds) and are set to +inf / cell 0 behind it.
//  - Packed keys: best and runner-up are kept as (bits of d2 & ~7) | candidate number 0..7 of the trip --
//    d2 >= +0, so the words order like the distances, the sentinels (>= 1.8e19) and kNoCand above every real candidate.  A
//    candidate is one v_and_or_b32, one v_med3_u32 and one v_min_u32; the leader's number is the key's low bits; within a
//    trip the number ascends with the cell index, so equal kept bits keep the first.  best32 / second32 leave without
//    their last three mantissa bits: the caller's band `tol` carries the term that covers them (see there).
constexpr float kNoCand = 1e18f;
template <typename MT, int WS>
__device__ __forceinline__ void nearest_rows_lean(const u64 *rm, const short *rs, const int nrows, const int wr, const float apf,
                                                  const float bpf, const int a_r, const MT lowm, const bool act,
                                                  float &best32, float &second32, int &bc)
{
    constexpr int MB = (int)sizeof(MT) * 8;
    auto rowmask = [&](int b) -> MT { return MB == 32 ? (MT)reinterpret_cast<const unsigned *>(rm)[2 * b] : (MT)rm[b]; };
    // lowest / highest set bit of a 32-bit word, 0xFFFFFFFF for zero (the plain builtins are undefined there)
    auto ffbl = [](unsigned v) -> unsigned { unsigned r; asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v)); return r; };
    auto ffbh = [](unsigned v) -> unsigned { unsigned r; asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(v)); return r; };
    auto sat = [](unsigned x, unsigned y) -> unsigned { return __builtin_elementwise_add_sat(x, y); };
    auto umed3 = [](unsigned x, unsigned y, unsigned z) -> unsigned { unsigned r; asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z)); return r; };
    int lead_b = 0;
    unsigned kb = __float_as_uint(best32), ks = __float_as_uint(second32);          // best and runner-up key (+inf on entry)
    auto cand_row = [&](int b, MT rowm, auto kc) {
        constexpr int k = decltype(kc)::value;
        const float dy = (float)b - bpf, dy2 = dy * dy;
        const MT up = rowm >> a_r, dn = rowm & lowm;
        unsigned fu, fd;                                         // first column of `up`, last of `dn` counted from the top bit
        if constexpr (MB == 32) { fu = ffbl((unsigned)up); fd = ffbh((unsigned)dn); }
        else {
            fu = min(ffbl((unsigned)up), sat(ffbl((unsigned)((u64)up >> 32)), 32u));
            fd = min(ffbh((unsigned)((u64)dn >> 32)), sat(ffbh((unsigned)dn), 32u));
        }
        const unsigned a_up = sat((unsigned)a_r, fu), a_dn = fd ^ (unsigned)(MB - 1);
        const float dxu = (float)a_up - apf, dxd = (float)a_dn - apf;
        const float d2u = fmaf(dxu, dxu, dy2), d2d = fmaf(dxd, dxd, dy2);
        // packed keys: a non-negative float orders like its bits, so (bits & ~7) | candidate number is one word that
        // carries distance and candidate; runner-up and best are one v_med3_u32 and one v_min_u32.  Lower cell index first:
        // within a trip equal kept bits keep the lower number (and every such tie is re-done exactly)
        const unsigned kd = (__float_as_uint(d2d) & ~7u) | (unsigned)(2 * k), ku = (__float_as_uint(d2u) & ~7u) | (unsigned)(2 * k + 1);
        ks = umed3(kb, ks, kd); kb = min(kb, kd);
        ks = umed3(kb, ks, ku); kb = min(kb, ku);
    };
    auto trip = [&](int b, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        const MT m0 = rowmask(b), m1 = (!TAIL || b + WS < nrows) ? rowmask(b + WS) : (MT)0;
        const MT m2 = (!TAIL || b + 2 * WS < nrows) ? rowmask(b + 2 * WS) : (MT)0;
        const unsigned kb_in = kb;
        cand_row(b, m0, std::integral_constant<int, 0>{}); cand_row(b + WS, m1, std::integral_constant<int, 1>{});
        cand_row(b + 2 * WS, m2, std::integral_constant<int, 2>{});
        if constexpr (!TAIL) cand_row(b + 3 * WS, rowmask(b + 3 * WS), std::integral_constant<int, 3>{});
        lead_b = kb < kb_in ? b : lead_b;
    };
    int b = wr;
    for (; b + 3 * WS < nrows; b += 4 * WS) trip(b, std::false_type{});
    if (b < nrows) trip(b, std::true_type{});
    const int lead = (int)(kb & 7u);
    best32 = __uint_as_float(kb & ~7u); second32 = __uint_as_float(ks & ~7u);
    const bool found = act && best32 < kNoCand;                  // (a split always has a row with a cell)
    const int lrow = found ? lead_b + (lead >> 1) * WS : 0;
    const MT below = rowmask(lrow) & lowm;
    const int lc = rs[lrow] + (MB == 32 ? __popc((unsigned)below) : __popcll((unsigned long long)below)) - 1 + (lead & 1);
    bc = found ? lc : 0;
    if (!act) { best32 = INFINITY; second32 = INFINITY; }
}

// The set columns of lattice row b within lattice distance rho of one agent, for the WALK_LEAN kernels (k_env, part 3): what
// the kernel's row_sel lambda answers, shifted down to the agent's first possible column c0 -- a 32-bit word, bit q = column
// c0 + q.  Both passes call it: the sensed radius with c0 = ca0 (the word is the window row as srow keeps it), the covered
// radius with a first column of its own.  Returns the columns that are in range for certain; `bnd` takes the (rare) boundary
// columns, which the caller puts to the reference's fp64 test on the stored cell.  MT: the row-mask word.
//  - The row word is shifted to c0 once, in front; everything behind it is 32-bit.  No column below c0 can be in range (c0 =
//    ceil(a - (rho + 2 lat_m)) clamped to 0..63, an interval starts at ceil(a - ho) with ho <= rho + lat_m), and the interval
//    ends less than 2 rho + 1 + 3 lat_m columns behind c0.  The host holds both radii to what the word takes
//    (classify_cells, env_api.hip): a set walks only if its sensed window is at most 15 rows (rho < 7.5: <= 16 columns
//    behind c0) and, on these kernels, its covered window at most 29 rows (rho_c < 14.49: < 30 columns behind c0, the
//    clamp of cmax at 30 cuts nothing); any other set takes the generic scan.
//  - Interval: ax = (float)(a - c0) is the agent's column coordinate relative to c0, the ends are ceil(ax - ho) and
//    floor(ax + ho) clamped to 0 and to cmax = min(ncols - 1 - c0, 30).  cmax < 0 (c0 behind the last column) and an interval
//    wholly left or right of the lattice give hi < lo: that empties the row word, with the lane and row tests, in one
//    select.  hi >= lo means 0 <= lo <= hi <= 30, so the range is 2 (1 << hi) - (1 << lo) and no shift is out of range
//    (the `& 31` only say so for the empty case, whose word is 0 whatever the range).
//  - Numerics: the bound documented above the lattice path holds with room to spare.  |ax| <= |a| (c0 lies between 0 and a's
//    window), so the cast error 2^-24 |ax| is at most that of the absolute coordinate, the column c - c0 is an exact small
//    integer, and fit tolerance and sqrt roundings are what they were: < 2e-5 steps against lat_m >= 1e-4.  Columns inside the
//    radius shrunk by lat_m (ri2) are in range for certain, columns outside the radius grown by lat_m (ro2) are not, and only
//    the two END columns can lie between: those are `bnd`.  An end that the clamp moved is tested like any other end
//    (lof / hif are the clamped ends).
//  - No callable parameter: a closure handed in here keeps the address of the kernel's argument struct alive until the
//    inliner is through, the struct is then copied field by field in the entry block, and the scalar registers of all 69
//    fields spill to lanes (594 lane reads in the headline kernel, +5.5 us: profiles/r25).
template <typename MT>
__device__ __forceinline__ unsigned row_sel_lean(const u64 *rm, const int nrows, const bool act, const int b, const float bpf,
                                                 const float ax, const int c0, const int cmax, const float ro2, const float ri2,
                                                 unsigned &bnd)
{
    constexpr int MB = (int)sizeof(MT) * 8;
    auto rowmask = [&](int q) -> MT { return MB == 32 ? (MT)reinterpret_cast<const unsigned *>(rm)[2 * q] : (MT)rm[q]; };
    const bool rowok = act && (unsigned)b < (unsigned)nrows;
    const int bq = b < 0 ? 0 : (b > 63 ? 63 : b);
    // read whatever the lane: all 64 entries of the table are written, and a read under a branch of its own would cut the
    // row's arithmetic into blocks (the clamp below then costs a canonicalising v_max in front of its own)
    const MT rowm = rowmask(bq);
    const float dy = (float)b - bpf, dy2 = dy * dy;
    const float ho2 = ro2 - dy2;
    // raw v_sqrt_f32 (1 ulp): its error is far inside the margin
    const float ho = __builtin_amdgcn_sqrtf(__builtin_amdgcn_fmed3f(ho2, 0.0f, INFINITY));
    const float f0 = ceilf(ax - ho), f1 = floorf(ax + ho);           // columns that may be in range, relative to c0
    // (the ends stay floats for their tests: no round trip through integers)
    const float lof = fmaxf(f0, 0.0f), hif = fminf(f1, (float)cmax);
    const int lo = (int)lof, hi = (int)hif;
    const float e0 = lof - ax, e1 = hif - ax;
    // one select empties the word: a lane or a row outside, no column at this row's height, or hi < lo
    const bool any_o = rowok && ho2 > 0.0f && hi >= lo;
    const unsigned wrow = any_o ? (unsigned)(rowm >> (c0 & (MB - 1))) : 0u;
    // an end column is certain when its own model distance is inside the shrunk radius
    const bool ok0 = fmaf(e0, e0, dy2) < ri2, ok1 = fmaf(e1, e1, dy2) < ri2;
    const unsigned bl = 1u << (lo & 31), bh = 1u << (hi & 31);                   // (hi >= lo: 0 <= lo, hi <= 30)
    const unsigned m = ((bh - bl) + bh) & wrow;                                  // columns lo .. hi of the row: 2 bh - bl
    bnd = ((ok0 ? 0u : bl) | (ok1 ? 0u : bh)) & m;                               // boundary columns: the caller's exact test
    return m ^ bnd;
}

// LAT: every env's target cells are a lattice subset (host-detected, KP::lattice) -- a compile-time switch, so that each
// instantiation carries ONE cell path and stays inside the 64 KB instruction cache: the row-space lattice walk, or the
// generic scan of all cells.
// FILT: one of the two launches of a mixed batch (KP::path_filter).  A template parameter and not a run-time test: any early
// exit, however cheap, changes how the generic kernel's scalar registers are spilled (+10 KB of lane reads at N = 64, past
// the instruction cache), so the kernels of unmixed batches are compiled without it and stay what they were.
//
// The kernel in order, and what ends each part ("barrier": __syncthreads; "lattice | generic" where the two paths differ):
//   1 prologue      the step's global loads; lattice row tables | fp32 cell copy -> LDS; split A: forces, integration, new
//                   state -> LDS and HBM.  Barrier: state, tables and cell copy are published.
//   2 pair pass     the threshold masks of every agent pair, dealt over the splits.  Barrier: the masks are complete.  Then
//                   split B alone: ordered neighbour insertion, contact spring of the next step -- beside the others' part 3.
//   3 walk | scan   sensed rows, covered columns and the walking splits' nearest-cell candidates | sensed words, occupied
//                   words (N <= 64) or per-cell ballots, every split's candidate.  Barrier: also publishes B's neighbour lists.
//   4 merge         nearest cell and in-shape flag, in every split alike; split A stores them.  No barrier of its own: the
//                   next one publishes them.
//   5 lattice tail  (K) kept rows, their counts, list fill: barrier.  (S) rank by list length: barrier.  (E) list emission
//                   and fp32 reward sums, each wave for its own sixteen agents: wave barrier.  (R) reward, inside the wave.
//                   Then part 7, no barrier.
//     generic tail  occupied-cell filter: barrier.  Clearing the rank-select bits: barrier.  Rank select: barrier (N > 64, or
//                   an agent over the cap).  List emission: the same barrier.  fp32 reward sums: barrier.  Verdict and
//                   reward on split A.
//   6 export        export launches only, split A (lattice: behind a barrier, the other waves' lists must be complete).
//   7 outputs       prior policy of the next step (split B), observation heads, sensed rows.  No barrier; the workgroup
//                   ends with its slowest wave.  The lattice kernel runs them at the end of part 5, ahead of part 6.
template <int NPAD, typename OT, bool DO_STEP, bool LAT, bool HALF = false, bool FILT = false>
__global__ void __launch_bounds__((Geo<NPAD, HALF>::T), (LAT ? Geo<NPAD, HALF>::WPS_LAT : Geo<NPAD, HALF>::WPS_GEN))
k_env(const KP P, const void *__restrict__ action, const int act_mode, OT *__restrict__ obs,
      float *__restrict__ reward, uint8_t *__restrict__ done, OT *__restrict__ a_prior)
{
    typedef Geo<NPAD, HALF> G_;
    constexpr int AG = G_::AG, EPB = G_::EPB, NW = G_::NW, WPE = G_::WPE, T = G_::T;
    constexpr int ACTW = G_::ACTW, LPA = G_::LPA, AGW = G_::AGW;
    static_assert(!HALF || LAT, "the half-occupied geometry exists for the lattice path only");
    static_assert(!HALF || !FILT, "the launches of a mixed batch use the full geometry");
    // ablation hooks (REPS / EXIT_AT): compiled out of the N = 64 lattice kernels of the full geometry -- the TGT_LDS kernels
    // below -- unless the library is a diagnostic build.  They sit at the 72-VGPR limit of seven workgroups per CU, and the
    // hooks cost them an SGPR pair held across the kernel, a run-time loop around every phase and twelve edges to the end.
    constexpr bool DIAG = kDiagBuild || !(LAT && NPAD == 64 && !HALF);
    // the same twelve kernels walk the lattice rows in fewer instructions (part 3): the nearest-cell loop takes empty sides by
    // a sentinel distance, four rows a trip and the winner's cell index once; an env picks the 32-bit walk by its own width;
    // split B leaves out the lattice coordinates that only the walking splits read; the window rows are 32-bit words relative
    // to the agent's first column from the start (row_sel_lean), best and runner-up packed keys (profiles/r25).  The switch
    // below exists for A/B builds (profiles/r18).
    constexpr bool WALK_LEAN = LAT && NPAD == 64 && !HALF;
#ifndef SWARM_WALK_ENV32
#define SWARM_WALK_ENV32 1                     // an env of <= 32 columns takes the 32-bit walk whatever the batch's widest (0: lat_n32 alone)
#endif
    typedef typename Pair<OT>::type OT2;

    extern __shared__ __align__(16) unsigned char smem[];
    // offset of LDS region r: the compile-time map (LatMap) on lattice launches of the geometries that gain from it
    // (Geo::CT_MAP), else layout_t's run-time offsets -- on lattice launches the same map, handed over in KP
    typedef LatMap<NPAD, HALF> LM;
#define LO(r) ((LAT && G_::CT_MAP) ? LM::r : P.off_##r)
    // The LDS views of BOTH paths, each tagged with the path that reads it: [both], [gen] = generic scan only, [lat] = lattice
    // walk only.  They stay here, in this order, one path's beside the other's: a view declared in the block that uses it
    // takes the load of its run-time offset out of the entry block, and the order in which the regions are first named
    // reaches the instruction schedule.  Tried view by view: the device code of every instantiation that reads the moved
    // view's offset at run time changes, and for the lattice views that of the compile-time map's instantiations as well.
    float *cxq = reinterpret_cast<float *>(smem + P.off_cxyf);          // [gen] fp32 cells, per PAIR {xa, xb, ya, yb} (pre-filter)
    double *sp = reinterpret_cast<double *>(smem + LO(sp));            // [both] [4][AG]: px, py, vx, vy
    u64 *cmask = reinterpret_cast<u64 *>(smem + P.off_cmask);            // [gen] [cell][NW]
    float *rsum = reinterpret_cast<float *>(smem + P.off_cmask);         // [gen] [WPE][3][AG]  (aliases cmask, later phase)
    unsigned *sbits = reinterpret_cast<unsigned *>(smem + P.off_sbits);  // [gen] [word][AG] sensed, then kept bits
    unsigned *obits = reinterpret_cast<unsigned *>(smem + P.off_obits);  // [gen] [word][AG] (export launches only)
    short *sidx = reinterpret_cast<short *>(smem + LO(sidx));          // [both] [AG][g_stride]
    typedef std::conditional_t<LAT, short, int> pc_t;                    // (lattice launches: 16-bit -- the kernel's LDS budget is seven workgroups per CU)
    pc_t *part_c = reinterpret_cast<pc_t *>(smem + LO(partc));         // [both] [WPE][AG] per-split nearest-cell candidates (cell index < 2^15)
    u64 *pm = reinterpret_cast<u64 *>(smem + LO(sidx));                // [both] [WPE][2 or 3][NW][AG] partial pair masks (aliases sidx, earlier phase)
    unsigned *owords = reinterpret_cast<unsigned *>(smem + P.off_cmask); // [gen] [word][AG] occupied bits (NW == 1; aliases cmask)
    short *snei = reinterpret_cast<short *>(smem + LO(snei));          // [both] [AG][kTopoMax]
    int *sncf = reinterpret_cast<int *>(smem + LO(sncf));              // [both] [AG]: nearest cell | in_flag<<30
    u64 *snear = reinterpret_cast<u64 *>(smem + LO(snear));            // [both] [NW][AG] nearby-agent masks
    u64 *lrm = reinterpret_cast<u64 *>(smem + LO(lat));                // [lat] [EPB][64] lattice row masks
    short *lrs = reinterpret_cast<short *>(smem + LO(lat) + (size_t)EPB * 64 * 8);   // [lat] [EPB][64] row starts
    int *sflag = reinterpret_cast<int *>(smem + LO(flag));             // [lat] per-lane exception flags, one BYTE per agent thread (flag_get below); generic launches: [AG] ints,
                                                                         // cleared in the prologue and unread by the generic kernel
    unsigned char *pc = smem + P.off_pc;                                 // [gen] [word][AG] kept-bit counts
    // row-space representation of the lattice path (LAT): window row t of agent thread `at` = lattice row b0 + t, its
    // columns are stored relative to the agent's first column ca0 (<= 17 columns are ever in range: 32-bit words)
    constexpr int NRC = LM::NRC;                                            // [lat] window rows stored per agent (lat_nrs <= 15)
    float4 *hdr = reinterpret_cast<float4 *>(smem + LO(hdr));          // [lat] [AG] {apr = a - ca0, bpr = b - b0, b0, ca0} (last two: ints)
    unsigned *srow = reinterpret_cast<unsigned *>(smem + LO(srow));    // [lat] [NRC][AG] sensed, then kept columns of window row t (17 bits) | cell index of the row's column ca0 << 17
    unsigned char *pcr = smem + LO(pcr);                               // [lat] [AG][NRC] kept cells per window row
    u64 *covrow = reinterpret_cast<u64 *>(smem + LO(cov));             // [lat] [EPB][64] columns within r_avoid/2 of ANY agent, per lattice row
    unsigned char *perm = smem + LO(perm);                             // [lat] [T/64][64] agent threads in ascending list length (per wave; aliases part_d, later phase)
    unsigned *orow = reinterpret_cast<unsigned *>(smem + P.off_orow);    // [lat] [NRC][AG] occupied columns (export launches only)

    // a mixed batch (KP::path_filter != 0) is two launches over the same grid: this workgroup belongs to the lattice launch
    // if every one of its envs has a lattice record (nrows > 0), else -- as a whole -- to the generic one.  Scalar loads and a
    // workgroup-uniform exit, ahead of the first LDS write and the first barrier.
    if constexpr (FILT) {
        bool any_zero = false;
        for (int k = 0; k < EPB; ++k) {
            const int ek = blockIdx.x * EPB + k;
            any_zero = any_zero || P.lat[ek < P.n_env ? ek : P.n_env - 1].nrows == 0;
        }
        if (any_zero == LAT) return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    STAMP(0);
    const int at = tid % AG;                 // agent thread
    // split: wave-uniform (AG is a multiple of 64), kept in an SGPR.  The roles rotate with the workgroup index: the
    // k-th wave of every workgroup lands on the same SIMD, and splits A / B carry extra sequential work (forces, prior,
    // ordered insertion, reward combine) -- rotating spreads that over the four SIMDs of a CU.
    const int sx = __builtin_amdgcn_readfirstlane((tid / AG + (int)blockIdx.x) % WPE);
    const int aw = at >> 6;                  // which 64-agent group of the environment
    // (lattice tail (K) only: this agent thread's byte of the exception flags.  Defined here and not beside its one call: there
    // it changes the device code of 66 of the 162 instantiations)
    auto flag_get = [&]() -> bool { return ((reinterpret_cast<const unsigned *>(sflag)[at >> 2] >> ((at & 3) * 8)) & 1u) != 0; };
    const bool thr_on = NPAD >= 64 || at < ACTW;         // (half-occupied geometry: agent threads ACTW..63 hold nothing)
    const int el = (NPAD < 64 && thr_on) ? at / NPAD : 0;
    const int i = NPAD < 64 ? at % NPAD : at;
    const int e = blockIdx.x * EPB + el;
    const int n_a = P.n_a;
    const bool act = thr_on && (e < P.n_env) && (i < n_a);
    const int es = e < P.n_env ? e : P.n_env - 1;
    const int ng = P.n_g[es];
    int ngb = ng;
    if (EPB > 1) {
        for (int k = 0; k < EPB; ++k) {
            const int ek = blockIdx.x * EPB + k;
            const int v = P.n_g[ek < P.n_env ? ek : P.n_env - 1];
            ngb = v > ngb ? v : ngb;
        }
    }
    const int W = (ngb + 31) >> 5;                       // target-cell words of this workgroup
    // Split roles: split 0 ("A") = forces / integration / reward combine; split SB ("B") = prior policy and
    // neighbour search, which run concurrently with A's work; every split scans target-cell words.  Words
    // [0, w0) belong to split B (it gets fewer), the rest are dealt round-robin to the other splits.
    constexpr int SB = WPE > 1 ? 1 : 0;
    int w0 = W;
    if (WPE > 1) { w0 = (W - 2 * (WPE - 1)) / WPE; w0 = w0 < 0 ? 0 : w0; }
    auto mine = [&](int w) -> bool {
        if (WPE == 1) return true;
        if (w < w0) return sx == SB;
        const int o = (w - w0) % (WPE - 1);            // o-th of the non-B splits
        return sx == (o < SB ? o : o + 1);
    };
    // exact (fp64) cell coordinates are read from global memory where they are needed (prior target, nearest-cell
    // merge, observation values, the rare exact fallbacks); the env's 8.7 KB of cells stay L1/L2 resident.
    const double2 *gce = P.cells_xy + (size_t)es * P.ng_max;
    auto cell64 = [&](int c) -> double2 { double2 g = gce[c < ng ? c : 0]; if (!(c < ng)) { g.x = kSentinel; g.y = kSentinel; } return g; };
    const float *cq_e = cxq + (size_t)el * P.cxq_stride;

    // ---- issue every global load of the step up front (their latency overlaps the cell staging)
    const size_t sbase = (size_t)es * 2 * n_a;
    double px = __builtin_nan(""), py = __builtin_nan(""), vx = 0.0, vy = 0.0;   // inactive lanes: NaN positions,
    double ax = 0.0, ay = 0.0;                                                    // every comparison is false
    double sf0x = 0.0, sf0y = 0.0;
    OT2 pri_now; pri_now.x = to_out<OT>(0.0); pri_now.y = to_out<OT>(0.0);
    const bool copy_prior = DO_STEP && P.with_prior && a_prior != nullptr;
    if (sx == 0 && act) {
        // the contact-spring force of THIS step (ENV:442-457 + CPP:735-815) is a function of the pre-integration positions
        // only: the previous pass evaluated it on exactly these positions, off its critical path, and left it in HBM
        if (DO_STEP) { const double2 sfl = P.sf_next[(size_t)e * n_a + i]; sf0x = sfl.x; sf0y = sfl.y; }
        px = P.p[sbase + i]; py = P.p[sbase + n_a + i];
        vx = P.dp[sbase + i]; vy = P.dp[sbase + n_a + i];
        if (DO_STEP) {
            // act_mode bit 0: doubles; bit 1: the reference's (2, n_a) component-major layout with the envs side by side on
            // the agent axis (the numpy API, ENV:487), else agent-major pairs [E][N][2]
            if (act_mode & 2) {
                const size_t a0 = (size_t)e * n_a + i, a1 = a0 + (size_t)P.n_env * n_a;
                if (act_mode & 1) { ax = ((const double *)action)[a0]; ay = ((const double *)action)[a1]; }
                else { ax = (double)((const float *)action)[a0]; ay = (double)((const float *)action)[a1]; }
            }
            else if (act_mode & 1) { const size_t ab = ((size_t)e * n_a + i) * 2; ax = ((const double *)action)[ab]; ay = ((const double *)action)[ab + 1]; }
            else { const float2 af = reinterpret_cast<const float2 *>(action)[(size_t)e * n_a + i]; ax = (double)af.x; ay = (double)af.y; }
            // the prior policy of THIS step (CPP:1061-1196 via ENV:605-624) is a function of the pre-integration state and
            // of the neighbour list / nearest cell of the previous observation: the previous launch evaluated it at its end,
            // where all of that sat in registers and LDS, and left it in HBM -- here it is only handed to the caller
            if (copy_prior) pri_now = reinterpret_cast<const OT2 *>(P.prior_next)[(size_t)e * n_a + i];
        }
    }
    // ---- generic (non-lattice) mode: stage an fp32 copy of the target cells (ENV: grid_center (2, n_g)) in LDS, laid
    // out per pair of cells {xa, xb, ya, yb} for packed arithmetic, padded with a sentinel (fp32: +inf).  The lattice
    // walk needs no cell coordinates except on its rare exact paths, which read the fp64 cells from global memory.
    if constexpr (!LAT)
    for (int rep = 0, reps = REPS(9); rep < reps; ++rep)
    for (int k = 0; k < EPB; ++k) {
        FENCE();
        const int ek0 = blockIdx.x * EPB + k;
        const int ek = ek0 < P.n_env ? ek0 : P.n_env - 1;
        const int ngk = P.n_g[ek];
        const double *gx = P.cells + (size_t)ek * 2 * P.ng_max;
        const double *gy = gx + P.ng_max;
        for (int c = tid; c < W * 32; c += T) {
            double2 g;
            g.x = c < ngk ? gx[c] : kSentinel;
            g.y = c < ngk ? gy[c] : kSentinel;
            float *q = cxq + (size_t)k * P.cxq_stride + (c >> 1) * 4 + (c & 1);
            q[0] = (float)g.x; q[2] = (float)g.y;
        }
    }
    // (the generic arm is a store nobody reads -- the generic kernel never looks at a flag; it stays, as the device code does)
    if (sx == 0) { if constexpr (LAT) { if ((at & 3) == 0) sflag[at >> 2] = 0; } else sflag[at] = 0; }
    if constexpr (LAT) {
        for (int q = tid; q < EPB * 64; q += T) {
            const int ek0 = blockIdx.x * EPB + (q >> 6);
            const LatEnv &Lq = P.lat[ek0 < P.n_env ? ek0 : P.n_env - 1];
            lrm[q] = Lq.rowmask[q & 63]; lrs[q] = Lq.rowstart[q & 63];
            covrow[q] = 0;                                                   // covered columns are OR-ed in
        }
        if (sx == WPE - 1) reinterpret_cast<uint4 *>(pcr)[at] = uint4{0u, 0u, 0u, 0u};   // rows past lat_nrs stay empty
    }
    // ---- forces + integration (split A): wall spring / damper + the contact spring the previous pass left in sf_next,
    // semi-implicit Euler; the other splits meanwhile initialise LDS, and ONE barrier publishes everything.
    double npx = px, npy = py, nvx = vx, nvy = vy;
    auto forces_integrate = [&]() {
        for (int rep = 0, reps = REPS(1); rep < reps; ++rep) {
            FENCE();
            const double sfx = sf0x, sfy = sf0y;                            // contact spring: evaluated by the previous pass (below)
            STAMP(8);
            double Fx = 1 * ax + sfx, Fy = 1 * ay + sfy;                       // ENV:638,640
            if (P.boundary) {                                                   // CPP:817-855, ENV:515-518
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
            STAMP(10);
            // ---- integration, ENV:643-652
            nvx = vx + (Fx / 1.0) * P.dt; nvy = vy + (Fy / 1.0) * P.dt;
            nvx = nvx < -P.vel_max ? -P.vel_max : (nvx > P.vel_max ? P.vel_max : nvx);
            nvy = nvy < -P.vel_max ? -P.vel_max : (nvy > P.vel_max ? P.vel_max : nvy);
            npx = px + nvx * P.dt; npy = py + nvy * P.dt;
            if (P.periodic) {                                                    // ENV:773-776
                if (npx < P.bx0) npx += 2 * P.w_half;
                if (npx > P.bx2) npx -= 2 * P.w_half;
                if (npy < P.by3) npy += 2 * P.h_half;
                if (npy > P.by1) npy -= 2 * P.h_half;
            }
        }
    };
    auto publish_new_state = [&]() {
        sp[at] = npx; sp[AG + at] = npy; sp[2 * AG + at] = nvx; sp[3 * AG + at] = nvy;
        if (DO_STEP && act) {                              // (the observation-only pass leaves the state as it is)
            P.p[sbase + i] = npx; P.p[sbase + n_a + i] = npy;
            P.dp[sbase + i] = nvx; P.dp[sbase + n_a + i] = nvy;
            if (copy_prior) store_nt(&reinterpret_cast<OT2 *>(a_prior)[(size_t)e * n_a + i], pri_now);
        }
    };
    // The contact spring came from the previous pass (sf_next), so the integration needs nobody else's position: split A goes
    // from its loads straight to the new state and publishes it -- one barrier, for every N (round 2 parked the old
    // positions in LDS for the contact loop: a wave barrier at N <= 64, two more workgroup barriers above).
    if (sx == 0) {
        STAMP(11);                                                        // (diagnostic builds: the state / action loads have landed)
        // the whole workgroup waits for these ~100 instructions: issue them ahead of the CU's other waves (-1.5 %; the
        // same for the wave with the longest lists in the list phase, or for every wave past it, gained nothing)
        __builtin_amdgcn_s_setprio(3);
        if (DO_STEP) forces_integrate();
        publish_new_state();
        __builtin_amdgcn_s_setprio(0);
        STAMP(12);
    }
    __syncthreads();
    STAMP(1);
    EXIT_AT(0);
    px = sp[at]; py = sp[AG + at];            // (the velocities are re-read from LDS where the prior policy needs them:
                                              // held in registers across the whole kernel they were spilled to scratch)
    STAMP(2);
    EXIT_AT(1);

    // ---- pairwise masks + neighbour search, CPP:77-100 + _get_focused CPP:628-698: the topo nearest agents with
    // norm < d_sen (self removed), ascending; and the "nearby" agent mask of the occupied-cell filter
    // (CPP:152-164: un-wrapped distance < d_sen + r_avoid/2, self included).  For N <= 64 the branch-free mask
    // pass is dealt over all splits (a quarter of the agents j each) and OR-combined through LDS; the ordered
    // insertion of the (few) candidates runs on split B.
    constexpr int JN = NPAD < 64 ? NPAD : 64;                   // lanes >= n_a hold NaN positions: never candidates
    const double *spx = sp + el * NPAD, *spy = sp + AG + el * NPAD;
    // every split evaluates 1/WPE of the agents j of each 64-agent group (branch-free, unrolled); the partial masks
    // are OR-combined through LDS so that every lane ends up with its complete "nearby" masks (split B also with the
    // candidate masks)
    u64 nearbyN[NW], candN[NW], cand1N[NW], cand2N[NW], hitN[NW] = {};
    // which split evaluates the contact spring of the next step: B, beside the others' walk (at N = 256 B's insertion over
    // four 64-agent groups looks like the long pole in the stamps, but giving the spring to split A's walkers measured +1.5 %)
    constexpr int CS = SB;
    {
        constexpr int JQ = JN / WPE;                  // agents j per split and 64-agent group
        static_assert(JQ * WPE == JN && JQ <= 32, "pair pass: JN must split evenly into <= 32 agents per split");
        constexpr int PMK = 4;                        // masks per agent: nearby, candidates, close candidates, contacts
        // One compare + one add-with-carry per test: the compare's lane mask is the carry-in of acc = 2 acc + carry, so
        // after the JQ agents of this split bit (JQ-1-q) of acc is the answer for agent q; reversed and shifted into
        // place (agent j = sx*JQ + q) at the end.
        unsigned a_nb[1], a_cd[1], a_c1[1], a_ht[1];       // N <= 64: this split's partial masks (N > 64 ORs each group into LDS at once)
        bool exc = false;
        auto place = [&](unsigned acc) -> u64 { return (u64)(__brev(acc) >> (32 - JQ)) << (sx * JQ); };
        for (int rep = 0, reps = REPS(2); rep < reps; ++rep) {
            FENCE();
            exc = false;
            // (N > 64: the loop over the 64-agent groups stays rolled -- unrolled, the pair pass alone was 20 KB of a kernel
            // that has to fit a 64 KB instruction cache)
#pragma unroll 1
            for (int w = 0; w < NW; ++w) {
                unsigned nb = 0, cd = 0, c1 = 0, ht = 0, c2 = 0, a_hi = 0;
                const double *qx = spx + w * 64 + sx * JQ, *qy = spy + w * 64 + sx * JQ;
                // (two agents j per 16-byte LDS read at an immediate offset -- as 8-byte reads the compiler pairs x with y in one
                // stride-64 read whose address costs a vector add per pair; the periodic variant is a second copy of the loop,
                // not a branch and a register copy per pair: 601 -> 574 us at 256 x 4096)
                auto pairs = [&](auto per_c) {
                    const bool PER = per_c;                              // a compile-time constant in the two copies of the lattice kernels
                    static_assert(JQ % 2 == 0, "pair pass: two agents per LDS read");
#pragma unroll
                    for (int q = 0; q < JQ; q += 2) {
                        const double2 x2 = *reinterpret_cast<const double2 *>(qx + q), y2 = *reinterpret_cast<const double2 *>(qy + q);
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            double rx = (h ? x2.y : x2.x) - px, ry = (h ? y2.y : y2.x) - py;
                            const double d2u = rx * rx + ry * ry;
                            double d2 = d2u;
                            if (PER) { wrap_rel(rx, ry, P.w_half, P.h_half); d2 = rx * rx + ry * ry; }
                            // nearby (CPP:161), its exception band, contact pairs of the NEXT step (ENV:442-457) on the un-wrapped
                            // distance; candidates (CPP:658) and close candidates on the wrapped one
                            if constexpr (NW > 2)         // with the wider pre-selection ring (N > 128: pays there)
                                pair_tests6(d2u, d2, P.c_near, P.c_near_hi, P.c_ball, P.c_sen, P.c_close, P.c_close2, nb, a_hi, ht, cd, c1, c2);
                            else
                                pair_tests5(d2u, d2, P.c_near, P.c_near_hi, P.c_ball, P.c_sen, P.c_close, nb, a_hi, ht, cd, c1);
                        }
                    }
                };
                if constexpr (LAT) { if (P.periodic) pairs(std::true_type{}); else pairs(std::false_type{}); }
                else pairs(P.periodic != 0);                 // (the generic-scan kernels are beyond the instruction cache as it is: one copy)
                exc = exc || (a_hi != nb);             // some agent is not "nearby" by a hair (see the occupied-cell filter)
                if constexpr (NPAD < 64) { a_nb[0] = nb; a_cd[0] = cd; a_c1[0] = c1; a_ht[0] = ht; }
                else if (rep == reps - 1) {
                    // N >= 64: a split's share of a 64-agent group is JQ = 16 agents -- exactly one 16-bit quarter of the
                    // group's mask word.  Each split stores its quarter (plain 2-byte store, no atomics, nothing to zero);
                    // behind the barrier a reader gets the whole 64-bit word with one load.
                    unsigned short *pq = reinterpret_cast<unsigned short *>(pm) + sx;
                    auto quarter = [](unsigned acc) -> unsigned short { return (unsigned short)(__brev(acc) >> 16); };
                    pq[((size_t)(0 * NW + w) * AG + at) * 4] = quarter(nb);
                    pq[((size_t)(1 * NW + w) * AG + at) * 4] = quarter(cd);
                    pq[((size_t)(2 * NW + w) * AG + at) * 4] = quarter(c1);
                    pq[((size_t)(3 * NW + w) * AG + at) * 4] = quarter(ht);
                    if constexpr (NW > 2) pq[((size_t)(4 * NW + w) * AG + at) * 4] = quarter(c2);
                }
            }
        }
        STAMP(14);
        if constexpr (LAT) { if (exc) atomicOr(reinterpret_cast<unsigned *>(sflag) + (at >> 2), 1u << ((at & 3) * 8)); }   // resolve the occupied-cell filter of this agent exactly
        if constexpr (NPAD < 64) {
            // N < 64 (several environments per wavefront, JQ < 16): every split stores its partial masks, the readers OR the
            // WPE copies
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                // bit position of agent j in the wave-wide masks = its lane (el*NPAD + j)
                const u64 nbm = place(a_nb[w]);
                pm[((sx * PMK + 0) * NW + w) * AG + at] = NPAD < 64 ? (nbm << (el * NPAD)) : nbm;
                pm[((sx * PMK + 1) * NW + w) * AG + at] = place(a_cd[w]);
                pm[((sx * PMK + 2) * NW + w) * AG + at] = place(a_c1[w]);
                pm[((sx * PMK + 3) * NW + w) * AG + at] = place(a_ht[w]);
            }
            __syncthreads();
            nearbyN[0] = 0; candN[0] = 0; cand1N[0] = 0; cand2N[0] = 0;
#pragma unroll
            for (int q = 0; q < WPE; ++q) nearbyN[0] |= pm[(q * PMK + 0) * AG + at];
            if (sx == SB) {
#pragma unroll
                for (int q = 0; q < WPE; ++q) { candN[0] |= pm[(q * PMK + 1) * AG + at]; cand1N[0] |= pm[(q * PMK + 2) * AG + at]; }
            }
            if (sx == SB) {
#pragma unroll
                for (int q = 0; q < WPE; ++q) hitN[0] |= pm[(q * PMK + 3) * AG + at];
                hitN[0] &= ~(1ull << i);                                       // k != i
            }
        } else {
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                nearbyN[w] = pm[(0 * NW + w) * AG + at]; candN[w] = 0; cand1N[w] = 0; cand2N[w] = 0;
                if (sx == SB) { candN[w] = pm[(1 * NW + w) * AG + at]; cand1N[w] = pm[(2 * NW + w) * AG + at]; cand2N[w] = pm[(4 * NW + w) * AG + at]; }
            }
            if (sx == CS) {
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    hitN[w] = pm[(3 * NW + w) * AG + at];
                    if (w == (i >> 6)) hitN[w] &= ~(1ull << (i & 63));         // k != i
                }
            }
        }
    }
    const u64 nearby1 = nearbyN[0];
    STAMP(15);
    EXIT_AT(2);
    if (NW > 1 && sx == SB) __builtin_amdgcn_s_setprio(2);     // N > 64: B's insertion is a chain of dependent operations over four groups
                                                                // of candidates -- issue it first, the walkers' independent work fills the gaps
    if (sx == SB) for (int rep = 0, reps = REPS(10); rep < reps; ++rep) {
        FENCE();
        bool collision = false;
        double nd[kTopoMax]; int nj[kTopoMax];
#pragma unroll
        for (int k = 0; k < kTopoMax; ++k) { nd[k] = INFINITY; nj[k] = -1; }
        u64 nearby[NW], cand[NW];
        {
            // candidates = agents within d_sen, self removed (CPP:672-676).  When at least `topo` of them are within
            // the smaller radius sqrt(c_close), the topo nearest all come from those (every other one is strictly
            // farther): insert only them -- same list, far fewer loop trips.
            u64 c1[NW]; int n1 = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) { nearby[w] = nearbyN[w]; cand[w] = candN[w]; c1[w] = cand1N[w]; }
            if (i < 64 * NW) { const u64 self = ~(1ull << (i & 63)); cand[NPAD <= 64 ? 0 : (i >> 6)] &= self; c1[NPAD <= 64 ? 0 : (i >> 6)] &= self; }
#pragma unroll
            for (int w = 0; w < NW; ++w) n1 += __popcll(c1[w]);
            const bool few = n1 >= P.topo;
            if constexpr (NW > 2) {             // second, wider ring before falling back to everything within d_sen
                u64 c2[NW]; int n2 = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) c2[w] = cand2N[w];
                if (i < 64 * NW) c2[i >> 6] &= ~(1ull << (i & 63));
#pragma unroll
                for (int w = 0; w < NW; ++w) n2 += __popcll(c2[w]);
                const bool some = n2 >= P.topo;
#pragma unroll
                for (int w = 0; w < NW; ++w) cand[w] = some ? c2[w] : cand[w];
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) cand[w] = few ? c1[w] : cand[w];
        }
        // pass B: the topo nearest candidates in ascending (distance, index) order.  Each candidate's exact fp64 squared
        // distance is turned into a sort key whose lowest 8 mantissa bits carry its index (non-negative doubles order like
        // their bit patterns), and the key ripples through a sorted 7-entry register list with one v_min_f64 + one
        // v_max_f64 per entry -- a third of the instructions of a compare-and-swap chain on (distance, index) pairs.  The
        // keys differ from the squared distances by < 256 ulp, so the order is the reference's (by norm = sqrt, monotonic)
        // unless two of the 7 smallest squared distances agree in all but those bits (a true tie and every pair whose
        // square roots could coincide included): such a lane -- the 7th entry guards the boundary of the list -- redoes its
        // insertion with the exact compare-and-swap chain on the norms below.
        double dmin = INFINITY;
        {
            double nk[kTopoMax + 1];
#pragma unroll
            for (int k = 0; k <= kTopoMax; ++k) nk[k] = INFINITY;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                u64 h = cand[w];
                while (h) {
                    const int jj = __ffsll((unsigned long long)h) - 1;
                    h &= h - 1;
                    double rx = spx[w * 64 + jj] - px, ry = spy[w * 64 + jj] - py;
                    if (P.periodic) wrap_rel(rx, ry, P.w_half, P.h_half);
                    const double cd = rx * rx + ry * ry;
                    dmin = fmin(dmin, cd);
                    double key = __builtin_bit_cast(double, (__builtin_bit_cast(u64, cd) & ~0xFFull) | (u64)(w * 64 + jj));
#pragma unroll
                    for (int k = 0; k <= kTopoMax; ++k) {
                        const double lo = fmin(nk[k], key);
                        key = fmax(nk[k], key);
                        nk[k] = lo;
                    }
                }
            }
            bool amb = false;
#pragma unroll
            for (int k = 0; k < kTopoMax; ++k) {
                const u64 kb = __builtin_bit_cast(u64, nk[k]), kn = __builtin_bit_cast(u64, nk[k + 1]);
                const bool fin = nk[k] < INFINITY;
                nj[k] = fin ? (int)(kb & 0xFFull) : -1;
                amb = amb || (fin && nk[k + 1] < INFINITY && ((kb ^ kn) >> 8) == 0);
            }
            if (__any(amb)) {                     // rare: the exact (distance, index) insertion, ascending j => ties keep the lower index first
                int xj[kTopoMax];
#pragma unroll
                for (int k = 0; k < kTopoMax; ++k) { nd[k] = INFINITY; xj[k] = -1; }
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    u64 h = amb ? cand[w] : 0;
                    while (h) {
                        const int jj = __ffsll((unsigned long long)h) - 1;
                        h &= h - 1;
                        double rx = spx[w * 64 + jj] - px, ry = spy[w * 64 + jj] - py;
                        if (P.periodic) wrap_rel(rx, ry, P.w_half, P.h_half);
                        // the reference sorts by the NORM (CPP:636-641): two squared distances a few ulp apart can round to the
                        // same sqrt and are then a tie (lower index first), so this path compares the norms themselves
                        double cd = sqrt(rx * rx + ry * ry); int cj = w * 64 + jj;
                        bool ins = false;                 // once the candidate is placed the tail only shifts: an entry
#pragma unroll                                            // carried down must pass equal distances (it was ahead of them)
                        for (int k = 0; k < kTopoMax; ++k) {
                            const bool sw = ins || cd < nd[k];
                            ins = sw;
                            const double td = nd[k]; const int tjj = xj[k];
                            nd[k] = sw ? cd : td; xj[k] = sw ? cj : tjj;
                            cd = sw ? td : cd;    cj = sw ? tjj : cj;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < kTopoMax; ++k) nj[k] = amb ? xj[k] : nj[k];
            }
        }
        STAMP(13);
        if constexpr (NW > 1) {
#pragma unroll
            for (int w = 0; w < NW; ++w) snear[w * AG + at] = nearby[w];
        }
#pragma unroll
        for (int k = 0; k < kTopoMax; ++k) {                      // CPP:459-491 collision test on the NEW list
            const bool used = k < P.topo && nj[k] >= 0;
            snei[at * kNeiStride + k] = (short)(used ? nj[k] : -1);
            if (P.export_small && act && k < P.topo) P.nei[((size_t)e * n_a + i) * P.topo + k] = used ? nj[k] : -1;
        }
        // collision <=> some listed neighbour is closer than r_avoid (CPP:472-487) <=> the NEAREST candidate is (the list is
        // sorted, and the nearest candidate is always listed)
        collision = dmin < P.c_avoid;
        snei[at * kNeiStride + kTopoMax] = (short)(collision ? 1 : 0);
    }
    if (sx == CS) {
        // ---- ball-to-ball contact spring of the NEXT step: ENV:442-457 (_get_dist_b2b) + CPP:735-815 (_sf_b2b_all), on the
        // positions just published.  Entry (i,k) = collide * d_edge * k_ball * (-(delta/d_center)), delta = p_k - p_i (wrapped
        // when periodic), d_center un-wrapped for every pair the reference evaluates (its numpy wrap only touches agent 0's
        // row, which the i>j loop never reads); summed over k in index order (CPP:799-807).  The colliding pairs (centre
        // distance < 2 size_a) are the contact masks of the pair pass.  (Which split: CS above.)
        double sfx = 0.0, sfy = 0.0;
        for (int rep = 0, reps = REPS(1); rep < reps; ++rep) {
            FENCE();
            sfx = 0.0; sfy = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                u64 h = hitN[w];
                while (h) {
                    const int kk = __ffsll((unsigned long long)h) - 1;
                    h &= h - 1;
                    const double dx = spx[w * 64 + kk] - px, dy = spy[w * 64 + kk] - py;
                    const double dc = sqrt(dx * dx + dy * dy);
                    const double de = fabs(dc - P.size2);
                    double wx = dx, wy = dy;
                    if (P.periodic) wrap_rel(wx, wy, P.w_half, P.h_half);
                    const double ux = wx / dc, uy = wy / dc;
                    sfx += 1.0 * de * P.k_ball * (-ux);
                    sfy += 1.0 * de * P.k_ball * (-uy);
                }
            }
        }
        if (act) P.sf_next[(size_t)e * n_a + i] = make_double2(sfx, sfy);
        if (NW > 1) __builtin_amdgcn_s_setprio(0);
    }
    STAMP(3);
    EXIT_AT(3);

    // ---- target-cell scan over this split's words, _get_target_grid_state CPP:858-908: first-minimum
    // nearest cell, sensed-cell bits (d < d_sen), and per cell the ballot of agents with d <= r_avoid/2
    // (CPP:183-186 inverted).
    // fp32 pre-filter: a decision is taken in fp32 only when the fp32 squared distance is outside a guard band
    // around its threshold (band = rigorous bound of the fp32 evaluation error for |coordinates| <= coord_lim);
    // otherwise the word / the argmin is re-evaluated in fp64 exactly as the reference does.
    const float pxf = (float)px, pyf = (float)py;
    const bool lane_far = act && !(fabs(px) <= (double)P.coord_lim && fabs(py) <= (double)P.coord_lim);
    const bool wave_exact = (P.force_exact != 0) || (__any(lane_far) != 0);
    float best32 = INFINITY, second32 = INFINITY; int bc = 0;
    const f2v pxx = {pxf, pxf}, pyy = {pyf, pyf};
    if constexpr (LAT) {
        // ---- lattice path.  Row b of the lattice holds the cells of columns rowmask[b]; the columns within
        // lattice distance rho of the agent form an interval.  Columns inside the radius shrunk by the margin lat_m
        // are in range for certain, columns outside the radius grown by lat_m are not; the (rare) columns in between
        // are decided by the reference's exact fp64 test on the stored coordinates.  lat_m = 5x the model's error
        // bound: per coordinate 2^-24 |coordinate| (fp32 cast of the fp64 lattice coordinate) + 1e-6 (lattice fit
        // tolerance of detect_lattice) + ~1e-6 (fp32 radius / sqrt roundings), i.e. < 2e-5 steps for |coordinate| <= 128.
        // The sets stay in ROW space: window row t of an agent is lattice row b0 + t, its in-range columns are kept as a
        // 32-bit word relative to the agent's first possible column ca0 (the window is <= 17 columns wide).
        // (split B does not walk and is not split 0: in the WALK_LEAN kernels it passes all of this by)
        if (!(WALK_LEAN && WPE > 1) || sx != SB) {
        const LatEnv &L = P.lat[es];
        const double apd =(px - L.ox) * L.uxi + (py - L.oy) * L.uyi;
        const double bpd = (px - L.ox) * L.vxi + (py - L.oy) * L.vyi;
        const float apf = (float)apd, bpf = (float)bpd;
        const int nrows = L.nrows, ncols = L.ncols;
        const float lat_m = fmaxf(1e-4f, 8e-7f * fmaxf(fabsf(apf), fabsf(bpf)));
        // first window row / first window column: no row below b0s and no column below ca0 can be in range (the interval
        // of a row starts at ceil(a - h) with h <= R + margin)
        const int b0s = (int)ceilf(bpf - (L.R + 2.0f * lat_m));
        int ca0 = (int)ceilf(apf - (L.R + 2.0f * lat_m));
        ca0 = ca0 < 0 ? 0 : (ca0 > 63 ? 63 : ca0);
        if (sx == 0) {
            float4 hq;
            hq.x = (float)(apd - (double)ca0); hq.y = (float)(bpd - (double)b0s);
            hq.z = __int_as_float(b0s); hq.w = __int_as_float(ca0);
            hdr[at] = hq;
        }
        const u64 *rm = lrm + el * 64;
        const short *rs = lrs + el * 64;
        // Rows are dealt over the splits other than B: B runs the ordered neighbour insertion meanwhile (about one
        // split's share of the walk), so no split is the straggler at the barrier that follows.
        constexpr int WS = WPE > 1 ? WPE - 1 : 1;
        const int wr = WPE > 1 ? (sx < SB ? sx : sx - 1) : 0;
        // The walk is instantiated for 32-bit row masks (every env's lattice has <= 32 columns: the reference's shapes
        // do) and for 64-bit ones.
        auto walk = [&](auto tag) {
        typedef decltype(tag) MT;
        constexpr int MB = (int)sizeof(MT) * 8;
        auto rowmask = [&](int b) -> MT { return MB == 32 ? (MT)reinterpret_cast<const unsigned *>(rm)[2 * b] : (MT)rm[b]; };
        auto popc = [](MT v) -> int { return MB == 32 ? __popc((unsigned)v) : __popcll((unsigned long long)v); };
        auto ffs0 = [](MT v) -> int { return (MB == 32 ? __ffs((unsigned)v) : __ffsll((unsigned long long)v)) - 1; };
        // columns lo..hi inclusive, 0 <= lo, hi <= MB-1; empty when hi < lo
        auto range = [](int lo, int hi) -> MT { return hi >= lo ? (MT)((~(MT)0 >> (MB - 1 - hi)) & (~(MT)0 << lo)) : (MT)0; };
        auto row_sel = [&](int b, float rho, double cut) -> MT {
            // columns of row b within lattice distance rho of (apf, bpf); exact test d2 < cut on the boundary columns
            // (the WALK_LEAN kernels use row_sel_lean instead)
            const bool rowok = act && b >= 0 && b < nrows;
            const float dy = (float)b - bpf, dy2 = dy * dy;
            const float ro = rho + lat_m, ri = rho - lat_m, ri2 = ri > 0.0f ? ri * ri : 0.0f;
            const float ho2 = ro * ro - dy2;
            const bool any_o = rowok && ho2 > 0.0f;
            // raw v_sqrt_f32 (1 ulp): its error is far inside the margin
            const float ho = __builtin_amdgcn_sqrtf(fmaxf(ho2, 0.0f));
            int ao0 = (int)ceilf(apf - ho), ao1 = (int)floorf(apf + ho);     // columns that may be in range
            ao0 = ao0 < 0 ? 0 : ao0; ao1 = ao1 > ncols - 1 ? ncols - 1 : ao1;
            const int bq = b < 0 ? 0 : (b > 63 ? 63 : b);
            const MT rowm = any_o ? rowmask(bq) : (MT)0;
            const int rst = rs[bq];
            // The margin is far below one lattice step (the in-range band of a row is < 0.06 columns wide), so only the two
            // END columns of the interval can sit in the uncertain band; every column between them is in range for certain.
            // An end column is certain when its own model distance is inside the shrunk radius.
            const float e0 = (float)ao0 - apf, e1 = (float)ao1 - apf;
            const bool c0 = fmaf(e0, e0, dy2) < ri2, c1 = fmaf(e1, e1, dy2) < ri2;
            MT acc = range(ao0, ao1);
            MT bnd = (MT)((c0 ? (MT)0 : (MT)1 << (ao0 & (MB - 1))) | (c1 ? (MT)0 : (MT)1 << (ao1 & (MB - 1)))) & acc & rowm;   // boundary columns
            acc &= ~bnd;
            while (__any(bnd != 0)) {
                if (bnd != 0) {
                    const int a = ffs0(bnd);
                    bnd &= bnd - 1;
                    const int c = rst + popc(rowm & (MT)(((MT)1 << a) - 1));
                    const double2 g = cell64(c);                             // the reference's test on the stored cell
                    const double ex = g.x - px, ey = g.y - py;
                    if (ex * ex + ey * ey < cut) acc |= (MT)1 << a;
                }
            }
            return rowm & acc;
        };
        for (int rep = 0, reps = REPS(3); rep < reps; ++rep) {
            FENCE();
            // rows b with |b - bpf| < rho + margin: the first is ceil(bpf - rho - margin), at most floor(2 (rho + margin)) + 1
            // of them (lat_nrs / lat_nrc: that count for the largest rho of any env)
            if constexpr (WALK_LEAN) {
                // row_sel_lean, above the kernel: the same columns as a word relative to the pass's first column c0, in fewer
                // instructions per row; its boundary columns take the reference's test on the stored cell here.  The cell
                // index is rowstart + the row's set columns below c0 + q; row mask and rowstart are read again for it, in
                // the rare branch, so the common path holds neither.
                auto lean_row = [&](int b, float ax, int c0, int cmax, float ro2, float ri2, double cut) -> unsigned {
                    unsigned bnd;
                    unsigned sel = row_sel_lean<MT>(rm, nrows, act, b, bpf, ax, c0, cmax, ro2, ri2, bnd);
                    while (__any(bnd != 0)) {
                        if (bnd != 0) {
                            const int q = __builtin_ctz(bnd);
                            bnd &= bnd - 1;
                            int br = b < 0 ? 0 : (b > 63 ? 63 : b);
                            asm volatile("" : "+v"(br));                         // (the addresses below are worked out here, not per row)
                            const int c = rs[br] + popc(rowmask(br) & (MT)(((MT)1 << (c0 + q)) - 1));   // c0 + q is a set column: < MB
                            const double2 g = cell64(c);
                            const double ex = g.x - px, ey = g.y - py;
                            if (ex * ex + ey * ey < cut) sel |= 1u << q;
                        }
                    }
                    return sel;
                };
                {
                    const float ax = (float)(apd - (double)ca0);                 // (hdr.x)
                    const int cm = ncols - 1 - ca0, cmax = cm > 30 ? 30 : cm;
                    const float ro = L.R + lat_m, ri = L.R - lat_m, ro2 = ro * ro, ri2 = ri > 0.0f ? ri * ri : 0.0f;
                    for (int t = wr; t < P.lat_nrs; t += WS)
                        srow[t * AG + at] = lean_row(b0s + t, ax, ca0, cmax, ro2, ri2, P.c_sen);
                }
                // the same walk with radius r_avoid/2: the env's "covered by any agent" columns, per lattice row.  The pass
                // has a first column of its own; its words go back to lattice columns for the OR.
                const int b0c = (int)ceilf(bpf - (L.Rc + 2.0f * lat_m));
                int ca0c = (int)ceilf(apf - (L.Rc + 2.0f * lat_m));
                ca0c = ca0c < 0 ? 0 : (ca0c > 63 ? 63 : ca0c);
                const float axc = (float)(apd - (double)ca0c);
                const int cmc = ncols - 1 - ca0c, cmaxc = cmc > 30 ? 30 : cmc;
                const float roc = L.Rc + lat_m, ric = L.Rc - lat_m, ro2c = roc * roc, ri2c = ric > 0.0f ? ric * ric : 0.0f;
                for (int t = wr; t < P.lat_nrc; t += WS) {
                    const unsigned selc = lean_row(b0c + t, axc, ca0c, cmaxc, ro2c, ri2c, P.c_occ);
                    const int bq = b0c + t < 0 ? 0 : (b0c + t > 63 ? 63 : b0c + t);     // selc == 0 outside the lattice
                    if (selc != 0) {                                             // (a set bit: ca0c + its place < MB)
                        if constexpr (MB == 32) atomicOr(reinterpret_cast<unsigned *>(&covrow[el * 64 + bq]), selc << (ca0c & 31));
                        else atomicOr(reinterpret_cast<unsigned long long *>(&covrow[el * 64 + bq]), (unsigned long long)selc << ca0c);
                    }
                }
            } else {
            for (int t = wr; t < P.lat_nrs; t += WS)
                srow[t * AG + at] = (unsigned)(row_sel(b0s + t, L.R, P.c_sen) >> ca0);
            // the same walk with radius r_avoid/2: the env's "covered by any agent" columns, per lattice row
            const int b0c = (int)ceilf(bpf - (L.Rc + 2.0f * lat_m));
            for (int t = wr; t < P.lat_nrc; t += WS) {
                const MT selc = row_sel(b0c + t, L.Rc, P.c_occ);
                const int bq = b0c + t < 0 ? 0 : (b0c + t > 63 ? 63 : b0c + t);         // selc == 0 outside the lattice
                if (selc != 0) {
                    if constexpr (MB == 32) atomicOr(reinterpret_cast<unsigned *>(&covrow[el * 64 + bq]), (unsigned)selc);
                    else atomicOr(reinterpret_cast<unsigned long long *>(&covrow[el * 64 + bq]), (unsigned long long)selc);
                }
            }
            }
            // nearest cell (CPP:858-908) from the lattice too: in row b the nearest cell is the set column closest to
            // the agent's column coordinate, on either side of it -- two candidates per row, rows dealt over the splits.
            // best / runner-up are tracked in lattice units; a runner-up within the model's error of the best sends the
            // lane to the exact scan below (cells further out on the same side of a row are >= 1 step^2 worse than that
            // side's candidate, so they are never a runner-up within tolerance).
            best32 = INFINITY; second32 = INFINITY; bc = 0;
            // split the row at the agent's column: `dn` = set columns left of it, `up` = right of it; the nearest
            // of each side is that side's only possible best or runner-up
            const int ar0 = (int)floorf(apf) + 1;
            const int a_r = ar0 < 0 ? 0 : (ar0 > MB - 1 ? MB - 1 : ar0);
            const MT lowm = (MT)(((MT)1 << a_r) - 1);                        // columns < a_r
            const int nr_hi = EPB == 1 ? nrows : 64;
            // candidates of row b: model distance^2 (lattice units) and cell index of the nearest set column on each side
            auto row_cands = [&](int b, float &d2d, float &d2u, int &c_dn) {
                const MT rowm = (EPB == 1 || b < nrows) ? rowmask(b) : (MT)0;
                const float dy = (float)b - bpf, dy2 = dy * dy;
                const MT up = rowm >> a_r, dn = rowm & lowm;
                const int a_up = a_r + ffs0(up);
                const int a_dn = MB - 1 - (MB == 32 ? __clz((int)dn) : __clzll((long long)dn));
                const float dxu = (float)a_up - apf, dxd = (float)a_dn - apf;
                d2u = (act && up != 0) ? fmaf(dxu, dxu, dy2) : INFINITY;
                d2d = (act && dn != 0) ? fmaf(dxd, dxd, dy2) : INFINITY;
                c_dn = rs[b] + popc(dn) - 1;                                 // the `up` candidate is cell c_dn + 1
            };
            // `no_cand`: a second32 at or above it means that no second candidate was seen (the sentinel walk below
            // gives a side without a set column a finite distance above it instead of +inf)
            // (switched by WALK_LEAN alone: a condition that also names MB here moves registers in the other 150 kernels)
            float no_cand = INFINITY;
            if constexpr (WALK_LEAN) no_cand = kNoCand;
            if constexpr (WALK_LEAN) {
                // the same candidates in fewer instructions per row: nearest_rows_lean, above the kernel
                nearest_rows_lean<MT, WS>(rm, rs, nrows, wr, apf, bpf, a_r, lowm, act, best32, second32, bc);
            } else
            for (int b = wr; b < nr_hi; b += WS) {
                float d2d, d2u; int c_dn;
                row_cands(b, d2d, d2u, c_dn);
                // lower cell index first: on an exact tie the strict compare keeps it (and the tie is re-done exactly)
                second32 = __builtin_amdgcn_fmed3f(best32, second32, d2d);
                bool lt = d2d < best32;
                best32 = lt ? d2d : best32; bc = lt ? c_dn : bc;
                second32 = __builtin_amdgcn_fmed3f(best32, second32, d2u);
                lt = d2u < best32;
                best32 = lt ? d2u : best32; bc = lt ? c_dn + 1 : bc;
            }
            // runner-up within the model's error of the best (|coordinate error| <= 2^-23 max(|a|, |b|) from the fp32
            // cast + 1e-6 lattice fit tolerance, in steps): decide among this split's candidates with the reference's
            // fp64 distances, first minimum in ascending cell order (rows ascending, left candidate before right).
            const float lat_dlt = 1.2e-7f * fmaxf(fabsf(apf), fabsf(bpf)) + 2e-6f;
            // (WALK_LEAN, packed keys: best32 and second32 arrive without their last three mantissa bits, each up to
            // 2^-20 of itself too low, and the candidate that leads is the first of those that agree in the kept bits.  The
            // test second - best <= tol then sees a difference up to 2^-20 best32 too large and a tol up to 2^-21 of
            // itself too small, and the true model minimum lies up to 2^-20 best32 above best32: 2^-19 second32 on top of
            // tol covers the three, so every lane the full-width test sends to the exact scan still goes, with a threshold
            // no lower.  Which term is the larger depends on where the agent stands, lat_dlt growing with its coordinates:
            // at lat_dlt's floor of 2e-6 the first up to about 12 steps from the shape, this one further out.)
            float tol_keys = 0.0f;
            if constexpr (WALK_LEAN) tol_keys = 0x1p-19f * second32;
            const float tol = 6.0f * sqrtf(second32) * lat_dlt + 1e-9f + tol_keys;
            const bool unc_min = act && (wave_exact || (second32 < no_cand && (second32 - best32) <= tol));
            if (__any(unc_min)) {
                if (unc_min) {
                    const float thr = wave_exact ? INFINITY : best32 + tol;
                    double bestd = INFINITY; int bcd = bc;
                    for (int b = wr; b < nr_hi; b += WS) {
                        float d2d, d2u; int c_dn;
                        row_cands(b, d2d, d2u, c_dn);
                        const bool td = d2d <= thr, tu = d2u <= thr && d2u < INFINITY;
                        if ((td && d2d < INFINITY) || tu) {
                            const double2 g0 = cell64((td && d2d < INFINITY) ? c_dn : 0), g1 = cell64(tu ? c_dn + 1 : 0);
                            const double e0x = g0.x - px, e0y = g0.y - py, e1x = g1.x - px, e1y = g1.y - py;
                            const double q0 = e0x * e0x + e0y * e0y, q1 = e1x * e1x + e1y * e1y;
                            if (td && d2d < INFINITY && q0 < bestd) { bestd = q0; bcd = c_dn; }
                            if (tu && q1 < bestd) { bestd = q1; bcd = c_dn + 1; }
                        }
                    }
                    bc = bcd;
                }
            }
        }
        };
        // (WALK_LEAN, one env per workgroup: the env's OWN column count picks the walk -- a batch with one wider shape
        // keeps the 32-bit walk for the others)
        if (sx != SB || WPE == 1) { if (P.lat_n32 || (WALK_LEAN && SWARM_WALK_ENV32 && ncols <= 32)) walk(0u); else walk((u64)0); }
        }
    } else {
    // ---- generic path: every split scans its words of the env's cells, then settles its nearest-cell candidate
    for (int rep = 0, reps = REPS(3); rep < reps; ++rep) {
    FENCE();
    best32 = INFINITY; second32 = INFINITY; bc = 0;
    for (int w = 0; w < W; ++w) {
        if (!mine(w)) continue;
        unsigned word = 0, rword = 0;
        int mlo = 0, mhi = 0;                 // lanes 0..31: ballot (lo, hi halves) of cell b = lane
        int bl = 0; const float best_in = best32;
        unsigned orw = 0;                     // NW == 1: reversed occupied-bit accumulator
        const unsigned nlo = (unsigned)nearby1, nhi = (unsigned)(nearby1 >> 32);
        u64 unc = 0;
        const float4 *cq = reinterpret_cast<const float4 *>(cq_e + w * 64);
        static_for<16>([&](auto prc) {
            constexpr int pr = decltype(prc)::value;
            const float4 q = cq[pr];                              // {xa, xb, ya, yb}
            const f2v gx = {q.x, q.y}, gy = {q.z, q.w};
            const f2v rx = gx - pxx, ry = gy - pyy;
            const f2v d2v = __builtin_elementwise_fma(rx, rx, ry * ry);   // packed: two cells per instruction
            static_for<2>([&](auto hc) {
                constexpr int hh = decltype(hc)::value;
                constexpr int b = 2 * pr + hh;
                const float d2 = hh ? d2v.y : d2v.x;
                second32 = __builtin_amdgcn_fmed3f(best32, second32, d2);
                const bool lt = d2 < best32;                     // strict: ties keep the earlier cell
                best32 = lt ? d2 : best32;
                bl = lt ? b : bl;                                // word-local index: an inline constant
                const u64 m_slo = __ballot(d2 < P.csen_lo), m_shi = __ballot(d2 < P.csen_hi);
                const u64 m_olo = __ballot(d2 < P.cocc_lo), m_ohi = __ballot(d2 < P.cocc_hi);
                rword = shl1_or_mask(rword, m_slo);
                if constexpr (NW == 1) {
                    // occupied for lane i  <=>  some NEARBY agent is within r_avoid/2 of this cell (CPP:161,185)
                    const unsigned t = ((unsigned)m_olo & nlo) | ((unsigned)(m_olo >> 32) & nhi);
                    orw = shl1_or_mask(orw, __ballot(t != 0));
                } else {
                    mlo = writelane_c<b>((int)(unsigned)m_olo, mlo);
                    mhi = writelane_c<b>((int)(unsigned)(m_olo >> 32), mhi);
                }
                unc |= (m_slo ^ m_shi) | (m_olo ^ m_ohi);
            });
        });
        word = __brev(rword);
        unsigned oword = __brev(orw);
        if (best32 < best_in) bc = w * 32 + bl;
        u64 mym = ((u64)(unsigned)mhi << 32) | (unsigned)mlo;
        if (unc != 0 || wave_exact) {                     // rare: redo this word exactly
            word = 0; oword = 0;
#pragma unroll 4
            for (int b = 0; b < 32; ++b) {
                const double2 g = cell64(w * 32 + b);
                const double rx = g.x - px, ry = g.y - py;
                const double d2 = rx * rx + ry * ry;
                if (d2 < P.c_sen) word |= 1u << b;
                const u64 m = __ballot(d2 < P.c_occ);
                if (lane == b) mym = m;
                if (NW == 1 && ((((unsigned)m & nlo) | ((unsigned)(m >> 32) & nhi)) != 0)) oword |= 1u << b;
            }
        }
        sbits[w * AG + at] = word;
        if constexpr (NW == 1) owords[w * AG + at] = oword;
        else if (lane < 32) cmask[(size_t)(w * 32 + lane) * NW + aw] = mym;
    }
    }
    {   // nearest cell of this split: unambiguous in fp32 unless the runner-up is within tolerance
        const float tol = P.min_tol_a * sqrtf(second32) + P.min_tol_b * second32 + 1e-9f;
        const bool unc_min = act && (wave_exact || (second32 < INFINITY && (second32 - best32) <= tol));
        if (__any(unc_min)) {
            const float thr = unc_min ? (wave_exact ? INFINITY : best32 + tol) : -1.0f;
            double bestd = INFINITY; int bcd = bc;
            for (int w = 0; w < W; ++w) {
                if (!mine(w)) continue;
                for (int b = 0; b < 32; ++b) {
                    const int cc = w * 32 + b;
                    const float rx = cq_e[(cc >> 1) * 4 + (cc & 1)] - pxf, ry = cq_e[(cc >> 1) * 4 + 2 + (cc & 1)] - pyf;
                    if (fmaf(rx, rx, ry * ry) <= thr || (wave_exact && unc_min)) {
                        const double2 g = cell64(w * 32 + b);
                        const double ex = g.x - px, ey = g.y - py;
                        const double d2 = ex * ex + ey * ey;
                        if (d2 < bestd) { bestd = d2; bcd = w * 32 + b; }     // ascending c: first minimum
                    }
                }
            }
            if (unc_min) bc = bcd;
        }
    }
    }
    part_c[sx * AG + at] = (pc_t)bc;
    double *part_d = reinterpret_cast<double *>(smem + LO(partd));     // [lat] [WPE - 1][AG] exact distance of each walking split's candidate (the list phase's `perm` reuses it)
    // TGT_LDS (the lattice kernels of 64 agents): the candidate's offset from the agent stays in registers past the merge, and
    // the split whose candidate wins publishes it in LDS (`tgt`, behind the barrier that ends (K)).  It is, bit for bit, the
    // target block of the agent's observation head and the prior policy's attraction vector -- the same cell, the same
    // position, the same subtraction -- so neither gathers the cell again.
    constexpr bool TGT_LDS = LAT && NPAD == 64 && !HALF;
    double2 *tgt = reinterpret_cast<double2 *>(smem + LM::tgt);          // [lat, TGT_LDS] [AG] nearest cell - own position (aliases part_d, later phase)
    double cand_x = 0.0, cand_y = 0.0;
    int win = 0;                                                         // TGT_LDS: the split whose candidate the merge picked
    if constexpr (LAT) {
        // each walking split evaluates the exact distance of ITS candidate here, before the barrier (the gather overlaps the
        // other waves' walk); the merge behind the barrier then compares values that sit in LDS instead of every split
        // gathering every candidate
        if (sx != SB || WPE == 1) {
            const double2 g = cell64(bc);
            const double ex = g.x - px, ey = g.y - py;
            part_d[(WPE > 1 && sx > SB ? sx - 1 : sx) * AG + at] = ex * ex + ey * ey;      // [walking split][AG]
            if constexpr (TGT_LDS) { cand_x = ex; cand_y = ey; }
        }
    }
    STAMP(16);
    EXIT_AT(4);
    __syncthreads();
    STAMP(17);
    // merge the splits' candidates exactly: (d2 in fp64, cell index) lexicographic minimum = first minimum
    double best = INFINITY; bc = 0;
    for (int rep = 0, reps = REPS(12); rep < reps; ++rep) {
    FENCE();
    best = INFINITY; bc = 0;
#pragma unroll
    for (int s = 0; s < WPE; ++s) {
        if (LAT && WPE > 1 && s == SB) continue;                     // split B does not walk
        const int c = part_c[s * AG + at];
        double d;
        if constexpr (LAT) d = part_d[(WPE > 1 && s > SB ? s - 1 : s) * AG + at];
        else { const double2 g = cell64(c); const double ex = g.x - px, ey = g.y - py; d = ex * ex + ey * ey; }
        if (d < best || (d == best && c < bc)) { best = d; bc = c; if constexpr (TGT_LDS) win = s; }
    }
    }
    const bool in_shape = act && best < P.c_in[es];                    // CPP:889
    const bool tgt_mine = TGT_LDS && win == sx;                        // (a lane mask: scalar registers across (K))
    if (sx == 0) {
        sncf[at] = bc | (in_shape ? (1 << 30) : 0);
        if (P.export_small && act) {
            P.near_cell[(size_t)e * n_a + i] = bc;
            P.in_flag[(size_t)e * n_a + i] = in_shape ? 1 : 0;
        }
    }
    STAMP(4);
    EXIT_AT(5);

    // ---- observation rows, CPP:102-137,274-306: the rows of this workgroup's environments are contiguous in HBM
    const int PPR = P.obs_dim >> 1;                  // pairs per row
    const int HP = 2 * (P.with_self + P.topo) + 2;   // head pairs: agent block + target pos/vel
    const int envs_here = (P.n_env - blockIdx.x * EPB) < EPB ? (P.n_env - blockIdx.x * EPB) : EPB;
    const int rows = envs_here * n_a;
    OT2 *out = reinterpret_cast<OT2 *>(obs) + (size_t)blockIdx.x * EPB * n_a * PPR;

    // ---- prior policy, calculateActionPrior / robotPolicy CPP:1061-1196: a function of the positions, velocities,
    // neighbour list and nearest cell of THIS observation -- exactly what the reference feeds it at the start of the
    // next step (ENV:605-624: pre-integration state, previous neighbor_index).  Split B evaluates it here, where all of
    // that sits in LDS, and leaves it in HBM for the next launch; the other splits write its share of the head pairs.
    auto prior_policy = [&]() {
    if (sx == SB && P.with_prior) {
        double qx = 0.0, qy = 0.0;
        double lx = 0.0, ly = 0.0;                       // agent_strategy 'llm': the Python twin (ENV:892-940), other repulsion gain
        {
            const int ncf = sncf[at];
            // target: own position when in shape (CPP:889-897) => zero attraction; else the nearest cell
            double tx = px - px, ty = py - py;
            if constexpr (TGT_LDS) { const double2 t = tgt[at]; if (!(ncf >> 30)) { tx = t.x; ty = t.y; } }      // the merge's winner: that cell - (px, py)
            else if (!(ncf >> 30)) { const double2 g = cell64(ncf & 0xFFFF); tx = g.x - px; ty = g.y - py; }
            const double dt_ = sqrt(tx * tx + ty * ty);
            if (dt_ > 0) { qx += P.pk_att * tx / dt_; qy += P.pk_att * ty / dt_; }
            lx = qx; ly = qy;
            double avx = 0.0, avy = 0.0; int cnt = 0;
#pragma unroll
            for (int k = 0; k < kTopoMax; ++k) {
                const int j = snei[at * kNeiStride + k];
                const bool used = j >= 0;
                const int tj = el * NPAD + (used ? j : 0);
                const double x = px - sp[tj], y = py - sp[AG + tj];
                const double d2n = x * x + y * y;
                if (used && d2n > 0 && d2n < P.c_avoid) {            // 0 < d < r_avoid (CPP:1150-1160), d = sqrt(d2n): sqrt is monotonic
                    const double d = sqrt(d2n);
                    const double ux = x / d, uy = y / d;
                    const double factor = P.pk_rep * (P.r_avoid / d - 1.0);
                    qx += factor * ux; qy += factor * uy;
                    if (P.llm) { const double fl = P.pk_llm * (P.r_avoid / d - 1.0); lx += fl * ux; ly += fl * uy; }
                }
                if (used) { avx += sp[2 * AG + tj]; avy += sp[3 * AG + tj]; ++cnt; }
            }
            if (cnt > 0) {
                avx /= cnt; avy /= cnt;
                const double sxv = P.pk_ali * (avx - sp[2 * AG + at]), syv = P.pk_ali * (avy - sp[3 * AG + at]);
                qx += sxv; qy += syv; lx += sxv; ly += syv;
            }
        }
        if (act) {
            OT2 o; o.x = to_out<OT>(clamp_ref(qx, -1.0, 1.0)); o.y = to_out<OT>(clamp_ref(qy, -1.0, 1.0));
            reinterpret_cast<OT2 *>(P.prior_next)[(size_t)e * n_a + i] = o;
            if (P.llm) { double2 u; u.x = clamp_ref(lx, -1.0, 1.0); u.y = clamp_ref(ly, -1.0, 1.0); P.act_next[(size_t)e * n_a + i] = u; }
        }
    }
    };

    auto head_blocks = [&](bool early) {
        for (int rep = 0, reps = REPS(7); rep < reps; ++rep) {
            FENCE();
            // The head of a row is NB = self + topo + 1 BLOCKS of four values {x, y, vx, vy}: [own state], the neighbours,
            // the target.  Lane = (row, block): one 16-byte store per lane, eight lanes cover a row's 128-byte head.  Every
            // value is (minuend - subtrahend): own block own - 0; neighbour k: neighbour - own (zeros without a neighbour,
            // CPP:79-81; the relative position wrapped when periodic, CPP:79); target: in shape own - own, else cell - own for
            // the position and 0 - own for the velocity (CPP:136-137).
            typedef OT OT4 __attribute__((ext_vector_type(4)));
            const int NB = P.with_self + P.topo + 1;
            // Who writes which blocks.  early == false (generic path): every split but B (busy with the prior policy) takes
            // items htid, htid + HT, ...  early == true (lattice path): the pass runs BEFORE the barrier that ends the list
            // phase -- it needs nothing from it -- on the two splits with the shortest lists there (A: five chunks of 64 items
            // out of eight, C: three), so that the split with the longest lists is not waited for twice.
            const int total = rows * NB;
            const bool b_out = WPE > 1 && P.with_prior != 0;
            const int HT = b_out ? T - AG : T;
            const int ps = tid / AG, ps_b = (SB + WPE - (int)(blockIdx.x % WPE)) % WPE;     // physical split index; split B's
            const int htid = b_out ? (ps < ps_b ? ps : ps - 1) * AG + at : tid;
            const int n_it = early ? (total + 63) >> 6 : (total + HT - 1) / HT;
            for (int it_ = 0; it_ < n_it; ++it_) {
                int item;
                if (early) {
                    const int c8 = it_ & 7, owner = c8 < 5 ? 0 : 2;
                    const int k = owner == 0 ? 5 * (it_ >> 3) + c8 : 3 * (it_ >> 3) + c8 - 5;      // the owner's k-th chunk
                    if (sx != owner || (k % NW) != aw) continue;
                    item = it_ * 64 + lane;
                } else {
                    if (b_out && sx == SB) break;
                    item = htid + it_ * HT;
                }
                if (item < total) {
                    const int r = NB == 8 ? item >> 3 : item / NB, blk = item - r * NB;
                    const int elr = EPB > 1 ? r / n_a : 0;
                    const int tr = elr * NPAD + (r - elr * n_a);
                    const double ox = sp[tr], oy = sp[AG + tr], ou = sp[2 * AG + tr], ov = sp[3 * AG + tr];
                    // straight-line code (every lane reads a neighbour slot, the nearest-cell word and that cell; the block kind
                    // only selects): a branch per kind would put each dependent LDS read / gather behind its own wait
                    const bool is_tgt = blk == NB - 1, is_nei = !is_tgt && !(P.with_self && blk == 0);
                    const int nslot = blk - P.with_self;
                    const int j = snei[tr * kNeiStride + (is_nei ? nslot : 0)];
                    const int ncf = sncf[tr];
                    const double2 g = P.cells_xy[(size_t)(blockIdx.x * EPB + elr) * P.ng_max + (ncf & 0xFFFF)];
                    const int tj = elr * NPAD + (j < 0 ? 0 : j);
                    const double nx = sp[tj], ny = sp[AG + tj], nu = sp[2 * AG + tj], nv = sp[3 * AG + tj];
                    const bool has = is_nei && j >= 0, out_t = is_tgt && !(ncf >> 30);
                    // minuend: neighbour | cell (target, outside the shape: velocity 0) | own; subtrahend: own | 0
                    const bool zero_m = is_nei && !has;
                    double mx = has ? nx : (out_t ? g.x : ox), my = has ? ny : (out_t ? g.y : oy);
                    double mu = has ? nu : (out_t ? 0.0 : ou), mv = has ? nv : (out_t ? 0.0 : ov);
                    if (zero_m) { mx = 0.0; my = 0.0; mu = 0.0; mv = 0.0; }
                    const bool sub_own = has || is_tgt;
                    const double qx = sub_own ? ox : 0.0, qy = sub_own ? oy : 0.0, qu = sub_own ? ou : 0.0, qv = sub_own ? ov : 0.0;
                    double a = mx - qx, b = my - qy;
                    if (P.periodic && is_nei) wrap_rel(a, b, P.w_half, P.h_half);
                    OT2 *dst = out + (size_t)r * PPR + 2 * blk;
                    if ((PPR & 1) == 0) {                                // rows are a whole number of blocks: 4-value stores stay aligned
                        const OT4 o = {to_out<OT>(a), to_out<OT>(b), to_out<OT>(mu - qu), to_out<OT>(mv - qv)};
                        __builtin_nontemporal_store(o, reinterpret_cast<OT4 *>(dst));
                    } else {                                             // odd list length (non-reference configs)
                        OT2 o0, o1;
                        o0.x = to_out<OT>(a); o0.y = to_out<OT>(b); o1.x = to_out<OT>(mu - qu); o1.y = to_out<OT>(mv - qv);
                        store_nt(dst, o0); store_nt(dst + 1, o1);
                    }
                }
            }
        }
    };

    // The same heads in the kernels that hold every agent's relative target in LDS (TGT_LDS): a writer of its own, so that
    // every other instantiation keeps head_blocks() and its code.  Same values, same stores, the early deal's chunks of 64
    // items; nothing is read from global memory, and the block kind selects ADDRESSES, not values.  A value is M - Q:
    //   own block        own - 0
    //   neighbour k      neighbour - own; no neighbour: own - own (+0 for every finite value: the reference's zeros)
    //   target           inside the shape own - own; outside: position tgt - 0, velocity 0 - own
    // M is one LDS read per value at `has ? neighbour : own` (positions of a target outside the shape: at its `tgt` entry);
    // Q is `own` or 0.  (Zeros are selected, never made by a product: (-0) - (-0) is not (-0) - 0.)  With eight blocks to a
    // row -- the reference's topology -- a lane's block and its kind are fixed over the chunks.
    // Chunks c of every eight: A takes [0, SWARM_HEAD_A), C the rest but the last SWARM_HEAD_B + SWARM_HEAD_D: B takes
    // SWARM_HEAD_B of them behind its prior, D the last SWARM_HEAD_D ahead of its rows
    // (5 / 3 / 0 / 0 as in head_blocks; 4 / 4, 4 / 3 / 1 and 5 / 2 / 1 measured the same: profiles/r16; with the straight-line
    // chunks 4 / 4 is 0.3 us behind and 3 / 3 / 0 / 2 1 us -- D has the longest lists: profiles/r17).
#ifndef SWARM_HEAD_A
#define SWARM_HEAD_A 5
#endif
#ifndef SWARM_HEAD_B
#define SWARM_HEAD_B 0
#endif
#ifndef SWARM_HEAD_D
#define SWARM_HEAD_D 0
#endif
    auto head_blocks_tgt = [&]() {
        static_assert(!TGT_LDS || (EPB == 1 && NW == 1), "one env per workgroup, row = agent thread");
        typedef OT OT4 __attribute__((ext_vector_type(4)));
        for (int rep = 0, reps = REPS(7); rep < reps; ++rep) {
            FENCE();
            const int NB = P.with_self + P.topo + 1;
            const int total = rows * NB, n_it = (total + 63) >> 6;
            auto owner = [](int it_) -> int { const int c8 = it_ & 7; return c8 < SWARM_HEAD_A ? 0 : (c8 < 8 - SWARM_HEAD_B - SWARM_HEAD_D ? 2 : (c8 < 8 - SWARM_HEAD_D ? SB : 3)); };
            // a wave without chunks leaves here: the set-up below and the induction registers of the chunk loop are vector
            // instructions too (about 80 per wave on B and D, which own nothing)
            if (!(sx == 0 || sx == 2 || (SWARM_HEAD_B > 0 && sx == SB) || (SWARM_HEAD_D > 0 && sx == 3))) continue;
            // block blk (of the kind the flags say) of row r, from its two index words: j, the neighbour slot (slot_of), and ncf
            // (plain: the caller has checked that the arena is not periodic and that rows are a whole number of blocks -- a
            // constant at each call, so that such a chunk is one basic block)
            auto slot_of = [&](const int r, const int blk, const bool is_nei) -> int { return snei[r * kNeiStride + (is_nei ? blk - P.with_self : 0)]; };
            auto emit = [&](const int r, const int blk, const bool is_self, const bool is_nei, const bool is_tgt, const bool plain,
                            const int j, const int ncf) {
                const bool has = is_nei && j >= 0, out_t = is_tgt && !(ncf >> 30);
                const int m = has ? j : r;
                const double *tq = reinterpret_cast<const double *>(tgt + r);
                const double *mpx = out_t ? tq : sp + m, *mpy = out_t ? tq + 1 : sp + AG + m;
                const double ox = sp[r], oy = sp[AG + r], ou = sp[2 * AG + r], ov = sp[3 * AG + r];
                const double mx = *mpx, my = *mpy, mu_ = sp[2 * AG + m], mv_ = sp[3 * AG + m];
                const bool q0 = is_self || out_t;
                const double qx = q0 ? 0.0 : ox, qy = q0 ? 0.0 : oy, qu = is_self ? 0.0 : ou, qv = is_self ? 0.0 : ov;
                const double mu = out_t ? 0.0 : mu_, mv = out_t ? 0.0 : mv_;
                double a = mx - qx, b = my - qy;
                if (!plain && P.periodic && is_nei) wrap_rel(a, b, P.w_half, P.h_half);
                OT2 *dst = out + (size_t)r * PPR + 2 * blk;
                if (plain || (PPR & 1) == 0) {                           // rows are a whole number of blocks: 4-value stores stay aligned
                    const OT4 o = {to_out<OT>(a), to_out<OT>(b), to_out<OT>(mu - qu), to_out<OT>(mv - qv)};
                    __builtin_nontemporal_store(o, reinterpret_cast<OT4 *>(dst));
                } else {                                                 // odd list length (non-reference configs)
                    OT2 o0, o1;
                    o0.x = to_out<OT>(a); o0.y = to_out<OT>(b); o1.x = to_out<OT>(mu - qu); o1.y = to_out<OT>(mv - qv);
                    store_nt(dst, o0); store_nt(dst + 1, o1);
                }
            };
            auto put = [&](const int r, const int blk, const bool is_self, const bool is_nei, const bool is_tgt) {
                emit(r, blk, is_self, is_nei, is_tgt, false, slot_of(r, blk, is_nei), sncf[r]);
            };
            if (NB == 8) {
                const int blk = lane & 7;
                const bool is_tgt = blk == 7, is_self = P.with_self && blk == 0, is_nei = !is_tgt && !is_self;
                if (!DIAG && rows == 64 && !P.periodic && (PPR & 1) == 0) {
                    // Every row of the env, the plain case, without the ablation hooks: the wave's chunks [F, F + C) are
                    // straight-line code -- no branch and no induction arithmetic between them, and nothing paid for the chunks
                    // of the other waves.  The index words of all of them are read first, so that the reads of a chunk's values
                    // are issued ahead of the previous chunk's conversion and store.
                    const int r0 = lane >> 3;
                    auto run = [&](auto first, auto count) {
                        constexpr int F = decltype(first)::value, C = decltype(count)::value;
                        int j[C > 0 ? C : 1], ncf[C > 0 ? C : 1];
                        static_for<C>([&](auto c) { constexpr int k = decltype(c)::value; const int r = (F + k) * 8 + r0; j[k] = slot_of(r, blk, is_nei); ncf[k] = sncf[r]; });
                        static_for<C>([&](auto c) { constexpr int k = decltype(c)::value; emit((F + k) * 8 + r0, blk, is_self, is_nei, is_tgt, true, j[k], ncf[k]); });
                    };
                    typedef std::integral_constant<int, SWARM_HEAD_A> nA;
                    typedef std::integral_constant<int, SWARM_HEAD_B> nB;
                    typedef std::integral_constant<int, SWARM_HEAD_D> nD;
                    typedef std::integral_constant<int, 8 - SWARM_HEAD_A - SWARM_HEAD_B - SWARM_HEAD_D> nC;
                    if (sx == 0) run(std::integral_constant<int, 0>{}, nA{});
                    else if (sx == 2) run(nA{}, nC{});
                    else if (sx == SB) run(std::integral_constant<int, 8 - SWARM_HEAD_B - SWARM_HEAD_D>{}, nB{});
                    else run(std::integral_constant<int, 8 - SWARM_HEAD_D>{}, nD{});
                } else {
                    // (a rolled loop: unrolled over the eight chunks behind their owner tests, with the hooks every TGT_LDS kernel
                    // takes 64 - 84 B of scratch, and without them it measures the same as the loop: profiles/r17)
                    for (int it_ = 0; it_ < n_it; ++it_) {
                        if (sx != owner(it_)) continue;
                        const int r = it_ * 8 + (lane >> 3);
                        if (r < rows) put(r, blk, is_self, is_nei, is_tgt);
                    }
                }
            } else {
                for (int it_ = 0; it_ < n_it; ++it_) {
                    if (sx != owner(it_)) continue;
                    const int item = it_ * 64 + lane;
                    if (item < total) {
                        const int r = item / NB, blk = item - r * NB;
                        const bool is_tgt = blk == NB - 1, is_self = P.with_self && blk == 0;
                        put(r, blk, is_self, !is_tgt && !is_self, is_tgt);
                    }
                }
            }
        }
    };

    // Exact exploration-reward verdict of ONE agent thread (CPP:529-549), wave-cooperative and called by the whole wave
    // with wave-uniform arguments: the 64 lanes evaluate one list slot each in fp64 -- psi needs a sqrt and a 12-term
    // cosine -- and the three sums then run over the lanes' values sequentially in slot order (v_readlane broadcasts), which
    // is the reference's order of additions.  Rare (the fp32 verdict decides outside its guard band); a lane looping alone
    // over its list made its workgroup a straggler.  La: agent thread, nL: its list length, eL: its environment.
    auto exact_uniform = [&](int La, int nL, int eL) -> bool {
        const double inv_dsen = 1.0 / P.d_sen;
        const double2 *gcl = P.cells_xy + (size_t)eL * P.ng_max;
        const double pxl = sp[La], pyl = sp[AG + La];
        const short *rowl = sidx + (size_t)La * P.g_stride;
        auto bcast = [](double v, int t) -> double {
            const u64 b = __builtin_bit_cast(u64, v);
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, t);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), t);
            return __builtin_bit_cast(double, ((u64)hi << 32) | lo);
        };
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int base = 0; base < nL; base += 64) {
            const int q = base + lane;
            double t0 = 0.0, t1 = 0.0, t2 = 0.0;
            if (q < nL) {
                const int cc = rowl[q];
                const double2 gq = gcl[cc];
                const double x = gq.x - pxl, y = gq.y - pyl;
                const double z = sqrt(x * x + y * y);
                // _rho_cos_dec(z, 0, d_sen), CPP:1012-1020; z < d_sen holds for every sensed cell
                const double psi = z < P.d_sen ? 0.5 * (1.0 + cospi01(z * inv_dsen)) : 0.0;
                t0 = psi * x; t1 = psi * y; t2 = psi;
            }
            const int m = nL - base < 64 ? nL - base : 64;
            for (int t = 0; t < m; ++t) { a0 += bcast(t0, t); a1 += bcast(t1, t); a2 += bcast(t2, t); }
        }
        if (a2 == 0) a2 = 1E-8;
        const double v0 = 1.0 * a0 / a2, v1 = 1.0 * a1 / a2;
        return sqrt(v0 * v0 + v1 * v1) < 0.05;
    };

    // The G sensed-cell pairs of the observation rows (CPP:274-291): value = stored cell - own position in f64, rounded once.
    // own == false (generic path, behind the workgroup barrier that completes every list): the waves deal the rows.
    // own == true (lattice path): every wave writes the rows of the sixteen agents whose lists IT has just emitted (pw: its
    // agent permutation) -- all four lanes of an agent sit in one wave, so no workgroup barrier separates list and rows.
    auto sensed_rows = [&](bool own, const unsigned char *pw) {
        for (int rep = 0, reps = REPS(8); rep < reps; ++rep) {
            FENCE();
            const int Gp = P.g_max;
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = T >> 6;
            // (N = 8: the wave's row slots through one pointer formed here -- the same bytes, and 12 to 20 B of scratch less in
            // those lattice kernels; at N = 32 that form measured 0.8 % slower, profiles/r14 and r15)
            const unsigned char *pws = !own ? pw : pw + (64 - ACTW) + sx * AGW;
            // row slot k of this wave -> agent thread tr, environment in the workgroup elr, output row r, "row exists"
            auto locate = [&](int k, int &tr, int &elr, int &r) -> bool {
                if (own) {
                    const int ta = (at & ~63) + (NPAD == 8 ? pws[k] : pw[(64 - ACTW) + sx * AGW + k]);
                    const int ii = NPAD < 64 ? (ta & 63) % NPAD : ta;
                    elr = NPAD < 64 ? (ta & 63) / NPAD : 0;
                    tr = ta; r = elr * n_a + ii;
                    return (blockIdx.x * EPB + elr) < P.n_env && ii < n_a;
                }
                r = k;
                const bool ok = r < rows;
                const int rq = ok ? r : rows - 1;
                elr = EPB > 1 ? rq / n_a : 0;
                tr = elr * NPAD + (rq - elr * n_a);
                return ok;
            };
            if (Gp == 80 && sizeof(OT) <= 4) {
                // the reference's list length: TWO slots per lane, so every store instruction writes 64 x 16 B (f32) of
                // consecutive addresses -- half the store instructions of the pair-per-lane form.  A row has 40 two-slot
                // chunks; 8 rows = 320 chunks = 5 full passes.
                typedef OT OT4 __attribute__((ext_vector_type(4)));
                const int ngrp = own ? AGW / 8 : (rows + nwv * 8 - 1) / (nwv * 8);
                for (int g8 = 0; g8 < ngrp; ++g8) {
#pragma unroll
                    for (int ps = 0; ps < 5; ++ps) {
                        const int ch = ps * 64 + lane;                   // 0..319
                        const int rl = (ch * 205) >> 13;                 // ch / 40 (exact for ch < 320)
                        const int m = ch - rl * 40;
                        // straight-line: both gathers of every pass are issued unconditionally (an empty slot reads cell 0
                        // and stores zeros), so the five passes' loads are in flight together instead of one wait each
                        int tr, elr, r;
                        const bool ok = locate(own ? g8 * 8 + rl : (wv + g8 * nwv) * 8 + rl, tr, elr, r);
                        const double2 *gr = P.cells_xy + (size_t)(blockIdx.x * EPB + elr) * P.ng_max;
                        const double qx = sp[tr], qy = sp[AG + tr];
                        const int cc = *reinterpret_cast<const int *>(sidx + (size_t)tr * P.g_stride + 2 * m);
                        const int c0 = (int)(short)(cc & 0xFFFF), c1 = cc >> 16;
                        const double2 g0 = gr[c0 < 0 ? 0 : c0], g1 = gr[c1 < 0 ? 0 : c1];
                        const OT z = to_out<OT>(0.0);
                        const OT a0 = to_out<OT>(g0.x - qx), b0 = to_out<OT>(g0.y - qy);
                        const OT a1 = to_out<OT>(g1.x - qx), b1 = to_out<OT>(g1.y - qy);
                        OT4 o = {c0 >= 0 ? a0 : z, c0 >= 0 ? b0 : z, c1 >= 0 ? a1 : z, c1 >= 0 ? b1 : z};
                        if (ok) __builtin_nontemporal_store(o, reinterpret_cast<OT4 *>(out + (size_t)r * PPR + HP + 2 * m));
                    }
                }
            } else {
                // any other list length / f64 rows: wave per row, lane = slot
                const int nrow = own ? AGW : (rows - wv + nwv - 1) / nwv;
                for (int k = 0; k < nrow; ++k) {
                    int tr, elr, r;
                    const bool ok = locate(own ? k : wv + k * nwv, tr, elr, r);
                    const double2 *gr = P.cells_xy + (size_t)(blockIdx.x * EPB + elr) * P.ng_max;
                    const double qx = sp[tr], qy = sp[AG + tr];
                    const short *srw = sidx + (size_t)tr * P.g_stride;
                    for (int q = lane; q < Gp; q += 64) {
                        const int c = srw[q];
                        const double2 g = gr[c < 0 ? 0 : c];
                        OT2 o; o.x = c >= 0 ? to_out<OT>(g.x - qx) : to_out<OT>(0.0); o.y = c >= 0 ? to_out<OT>(g.y - qy) : to_out<OT>(0.0);
                        if (ok) store_nt(&out[(size_t)r * PPR + HP + q], o);
                    }
                }
            }
        }
    };

    // The same rows in the lattice kernels of 64 agents (ROWS_LIVE; g_max == 80, rows of at most 4-byte elements): a writer
    // of its own, so that every other instantiation keeps sensed_rows() and its code as they are.  Same values, same
    // stores, another order; only passes that hold a cell do the work.
    //   Slot-aligned passes.  A wave's sixteen rows are two groups of eight, in its permutation's order: ascending list
    // length.  In a group, lane = 8 * row + column: pass p is slots [16 p, 16 p + 16) of the group's eight rows, 8 lanes x
    // 16 B (f32) of consecutive addresses per row.  Everything that belongs to a row -- permutation byte, position, list
    // address, store address -- is computed once per group; a pass adds constants, which sit in the instructions' offsets.
    //   Live and dead passes.  The group's longest list is its last agent's (nmax, capped); passes p >= ceil(nmax / 16) hold
    // no cell in any of the eight rows (the list region beyond a list's end is -1): they store zeros and read nothing.
    // `live` carries the two groups' live-pass counts, four bits each, taken on the scalar side in the reward block.
    //   The live passes of a group are a pipeline as before (profiles/r14): list words and gathers of up to four passes in
    // flight (bf16 rows: three), subtract / convert / select / store behind COUNTED waits, the gathers of pass t + 4 ahead of
    // the store of pass t.  One statically unrolled pipeline per live-pass count, picked by a scalar switch, run once per
    // group -- a group's fill is not overlapped with the other's drain.  A wave-uniform branch around a
    // load INSIDE one pipeline would make every wait behind it a full one.  The zero stores go behind the group's first
    // gathers: younger than those, they are in no gather's wait, and they fill the time the first gathers take.
    //   Nothing on the load path depends on "row exists" (n_a < 64): such a row reads cell 0 and only its stores are
    // predicated; a workgroup whose every row exists takes the twin without predicates.
    constexpr bool ROWS_LIVE = LAT && NPAD == 64 && !HALF && sizeof(OT) <= 4;
    auto sensed_rows_live = [&](const int live) {
        typedef OT OT4 __attribute__((ext_vector_type(4)));
        typedef std::integral_constant<bool, true> pred_yes;
        typedef std::integral_constant<bool, false> pred_no;
        // NP passes of 16 slots: g_max == 80.  DEPTH passes in flight; the bf16 rows' conversion takes registers of its own
        constexpr int S = (int)sizeof(OT2), DEPTH = sizeof(OT) == 2 ? 3 : 4, NP = 5;
        static_assert(!ROWS_LIVE || (EPB == 1 && AG == 64), "one env per workgroup, row = agent thread");
        for (int rep = 0, reps = REPS(8); rep < reps; ++rep) {
            FENCE();
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            const unsigned char *pws = perm + wv * 64 + (64 - ACTW) + sx * AGW;
            const char *gbase = reinterpret_cast<const char *>(P.cells_xy + (size_t)blockIdx.x * P.ng_max);
            const unsigned row_b = PPR * S, head_b = HP * S, list_b = P.g_stride * 2;
            auto group = [&](auto PRED, auto LIVE, const int g) {
                constexpr bool pred = decltype(PRED)::value;
                constexpr int L = decltype(LIVE)::value, F = L < DEPTH ? L : DEPTH;
                const int ta = pws[g * 8 + (lane >> 3)], col = lane & 7;  // the row's agent thread; the lane's two-slot column in a pass
                const bool ok = !pred || ((int)blockIdx.x < P.n_env && ta < n_a);
                char *dst = reinterpret_cast<char *>(out) + (__umul24(ta, row_b) + (head_b + col * (2 * S)));
                const OT z = to_out<OT>(0.0);
                auto gather = [&](int cc, double2 &g0, double2 &g1) {
                    const int c0 = (int)(short)(cc & 0xFFFF), c1 = cc >> 16;
                    g0 = *reinterpret_cast<const double2 *>(gbase + ((unsigned)(c0 < 0 ? 0 : c0) << 4));
                    g1 = *reinterpret_cast<const double2 *>(gbase + ((unsigned)(c1 < 0 ? 0 : c1) << 4));
                };
                auto put = [&](int p, OT4 o) {
                    OT4 *d = reinterpret_cast<OT4 *>(dst + p * (16 * S));
                    if constexpr (pred) { if (ok) __builtin_nontemporal_store(o, d); }
                    else __builtin_nontemporal_store(o, d);
                };
                if constexpr (L == 0) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) put(p, OT4{z, z, z, z});
                } else {
                    const char *lp = reinterpret_cast<const char *>(sidx) + (__umul24(ta, list_b) + col * 4);
                    auto word = [&](int p) -> int {
                        int cc = *reinterpret_cast<const int *>(lp + p * 32);
                        if constexpr (pred) {
                            asm volatile("" : "+v"(cc));                 // (the list word is read whether the row exists or not)
                            if (!ok) cc = -1;                            // no row: both gathers read cell 0
                        }
                        return cc;
                    };
                    const double qx = sp[ta], qy = sp[AG + ta];
                    int cc[DEPTH];
                    double2 ga[DEPTH], gb[DEPTH];
#pragma unroll
                    for (int t = 0; t < F; ++t) cc[t] = word(t);
#pragma unroll
                    for (int t = 0; t < F; ++t) gather(cc[t], ga[t], gb[t]);
                    __builtin_amdgcn_sched_barrier(0);                   // the first gathers stay ahead of the zero stores and of the first wait
#pragma unroll
                    for (int p = L; p < NP; ++p) put(p, OT4{z, z, z, z});
                    if constexpr (L < NP) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < L; ++t) {
                        const int k = t % DEPTH;
                        const bool more = t + DEPTH < L;
                        int cn = 0;
                        if (more) cn = word(t + DEPTH);
                        // predicated stores: the gathered values are "used" here, outside the branch, so the loads stay put
                        if constexpr (pred) asm volatile("" : "+v"(ga[k].x), "+v"(ga[k].y), "+v"(gb[k].x), "+v"(gb[k].y));
                        const int c0 = (int)(short)(cc[k] & 0xFFFF), c1 = cc[k] >> 16;
                        const OT a0 = to_out<OT>(ga[k].x - qx), b0 = to_out<OT>(ga[k].y - qy);
                        const OT a1 = to_out<OT>(gb[k].x - qx), b1 = to_out<OT>(gb[k].y - qy);
                        const OT4 o = {c0 >= 0 ? a0 : z, c0 >= 0 ? b0 : z, c1 >= 0 ? a1 : z, c1 >= 0 ? b1 : z};
                        if (more) { cc[k] = cn; gather(cn, ga[k], gb[k]); }
                        put(t, o);
                    }
                }
            };
            auto groups = [&](auto PRED) {
#pragma unroll 1
                for (int g = 0; g < AGW / 8; ++g) {
                    switch ((live >> (4 * g)) & 15) {
                    case 0: group(PRED, std::integral_constant<int, 0>{}, g); break;
                    case 1: group(PRED, std::integral_constant<int, 1>{}, g); break;
                    case 2: group(PRED, std::integral_constant<int, 2>{}, g); break;
                    case 3: group(PRED, std::integral_constant<int, 3>{}, g); break;
                    case 4: group(PRED, std::integral_constant<int, 4>{}, g); break;
                    default: group(PRED, std::integral_constant<int, NP>{}, g); break;
                    }
                }
            };
            if (n_a == NPAD && (int)blockIdx.x < P.n_env) groups(pred_no{});
            else groups(pred_yes{});
        }
    };
    int row_live = 0;                               // ROWS_LIVE: live passes of the wave's two row groups (sensed_rows_live)

    const int G = P.g_max;
    int n_sel = 0;                                   // length of this agent thread's capped list
    bool uniform = false, unsure = false;            // split A: fp32 verdict of the exploration reward / "redo it exactly"
    if constexpr (LAT) {
    // ================================================================================================================
    // Lattice path, row space.  After the walk every (window row t, agent) holds its sensed columns as a 32-bit word
    // relative to the agent's column ca0, and covrow[b] holds the env's covered columns of lattice row b.
    // (K) kept = in_shape ? sensed & ~covered : sensed (CPP:150,209-216), the row's first cell index and its kept count,
    //     rows dealt over the splits;  (S) the agent threads of each 64-group are ranked by list length;  (E) list
    //     emission + the fp32 reward sums in ONE walk over the kept bits, four lanes per agent (rank ranges), sixteen agents
    //     of SIMILAR list length per wave -- a wave loops as long as its longest range, so grouping by length is what turns
    //     the per-wave trip count from max(n) / 4 into (roughly) the quartile's n / 4.
    // ================================================================================================================
    const float4 hq = hdr[at];
    const int hb0 = __float_as_int(hq.z), hca0 = __float_as_int(hq.w);
    const LatEnv &L = P.lat[es];
    const u64 *rm = lrm + el * 64;
    const short *rs = lrs + el * 64;
    const bool flg = flag_get();                     // a pair within 1e-9 of the "nearby" threshold: exact occupied test
    for (int rep = 0, reps = REPS(4); rep < reps; ++rep) {
        FENCE();
        for (int t = sx; t < P.lat_nrs; t += WPE) {
            const int b = hb0 + t;
            const int bq = b < 0 ? 0 : (b > 63 ? 63 : b);
            const unsigned sel = srow[t * AG + at] & 0x1FFFFu;           // empty outside the lattice / for inactive lanes (the mask: REPS reruns)
            const u64 rowm = rm[bq];
            const int base = rs[bq] + __popcll(rowm & ((1ull << hca0) - 1ull));   // cell index of the first set column >= ca0
            unsigned kept = sel;
            if (in_shape) {
                // occupied <=> within r_avoid/2 of ANY agent: the covering agent of a SENSED cell is "nearby" (CPP:161) by
                // the triangle inequality, except when its distance sits within rounding of the nearby threshold -- those
                // lanes were flagged by the pair pass and are resolved with the reference's nearby x cell test.
                const unsigned cv = (unsigned)(covrow[el * 64 + bq] >> hca0);
                kept = sel & ~cv;
                if (flg) {
                    const unsigned relm = (unsigned)(rowm >> hca0);
                    unsigned it = sel & cv;
                    kept = sel;
                    while (it) {
                        const int c = __ffs(it) - 1; it &= it - 1;
                        const double2 g = cell64(base + __popc(relm & ((1u << c) - 1u)));
                        bool occ = false;
                        for (int q = 0; q < NW && !occ; ++q) {
                            u64 nbm = NW == 1 ? (nearby1 >> (NPAD < 64 ? el * NPAD : 0)) : snear[q * AG + at];
                            while (nbm && !occ) {
                                const int j = q * 64 + __ffsll((unsigned long long)nbm) - 1; nbm &= nbm - 1;
                                const double ex = g.x - spx[j], ey = g.y - spy[j];
                                occ = ex * ex + ey * ey < P.c_occ;
                            }
                        }
                        if (occ) kept &= ~(1u << c);
                    }
                }
            }
            if (rep == reps - 1) srow[t * AG + at] = kept | ((unsigned)base << 17);     // <= 17 window columns, cell index < 2^15
            pcr[at * NRC + t] = (unsigned char)__popc(kept);
            if (P.export_idx) orow[t * AG + at] = sel & ~kept;
        }
    }
    // unused list slots read -1 (CPP:46-50): the whole list region is filled here, the emission overwrites its slots
    {
        uint4 *fill = reinterpret_cast<uint4 *>(sidx);
        const int n16 = (AG * P.g_stride * 2) >> 4;
        for (int q = tid; q < n16; q += T) fill[q] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    }
    __syncthreads();
    STAMP(5);
    EXIT_AT(6);
    // every split is past its merge: the distances are dead, and the winning split's lane publishes the agent's relative
    // target over them (read by the prior policy and the heads, behind the next barrier)
    if constexpr (TGT_LDS) { if (tgt_mine) tgt[at] = double2{cand_x, cand_y}; }

    // ---- (S) rank of every agent thread by (list length, index) inside its 64-group: each split compares against a quarter
    // of the group (the other agents' keys come from the wave's own lanes), the partial counts are summed through LDS
    pc_t *prk = part_c;                                  // [WPE][AG] (the nearest-cell candidates are consumed)
    int n_kept;
    {
        const uint4 cq = reinterpret_cast<const uint4 *>(pcr)[at];
        n_kept = (int)__builtin_amdgcn_sad_u8(cq.x, 0u, __builtin_amdgcn_sad_u8(cq.y, 0u, __builtin_amdgcn_sad_u8(cq.z, 0u, __builtin_amdgcn_sad_u8(cq.w, 0u, 0u))));
        const int key = (lane < ACTW) ? n_kept * 64 + lane : lane - 64;      // empty agent threads first, in lane order
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) cnt += (__builtin_amdgcn_readlane(key, sx * 16 + q) < key) ? 1 : 0;
        prk[sx * AG + at] = (pc_t)cnt;
    }
    n_sel = n_kept > G ? G : n_kept;
    __syncthreads();
    STAMP(18);
    EXIT_AT(7);
    int ea;                                              // the agent thread this lane works for in (E)
    {
        int rank = 0;
#pragma unroll
        for (int s = 0; s < WPE; ++s) rank += prk[s * AG + at];
        unsigned char *pw = perm + (tid >> 6) * 64;      // this wave's own copy: no workgroup barrier needed
        pw[rank] = (unsigned char)lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // LPA lanes per agent, AGW agents per wave: split 0 takes the shortest lists, split 3 the longest
        ea = (at & ~63) + pw[(64 - ACTW) + sx * AGW + lane / LPA];
    }
    // No workgroup barrier follows: the workgroup ends with its slowest wave.  Issue priority by the work that is left -- split D
    // took the longest lists, C the next, B has the prior policy to run (D 3 / C 2 / B 1 / A 0).  N = 256, one workgroup per CU
    // and nothing else to fill a tail: 566 -> 550 us at 256 x 4096 (against 2/0/1: 558, 3/1/2: 555, 2/0/2: 561).  With seven
    // workgroups per CU at N = 64 it still pays: 83.9 -> 83.3 us; 32 x 1024 (one workgroup generation): 25.0 -> 24.35 us.
    { if (sx == 3) __builtin_amdgcn_s_setprio(3); else if (sx == 2) __builtin_amdgcn_s_setprio(2); else if (sx == SB) __builtin_amdgcn_s_setprio(1); }

    // ---- (E) capped sensed list (CPP:236-271) + exploration-reward sums (CPP:494-551), fp32 fast path.  The kept list of
    // an agent is cut into four contiguous RANK ranges, one per lane of its quad; each lane walks its range bit by bit
    // through the window rows.  Per kept cell: its list slot, its cell index (row base + set columns of the row mask
    // below it) and its reward weight psi(u), u = (distance / d_sen)^2 from the LATTICE coordinates -- |v| is invariant
    // under the lattice's rotation, so the sums run in lattice steps and need neither the stored cells nor a list
    // read-back.  The fp32 result only DECIDES outside a guard band; inside it the sums are redone in fp64 below.
    // LIST_LEAN (the lattice kernels of 64 agents, full geometry): the walk of a range is list_walk_lean, above the kernel.
    constexpr bool LIST_LEAN = LAT && NPAD == 64 && !HALF;
    float qn0 = 0.0f, qn1 = 0.0f, qdn = 0.0f, qrl = 1.0f; int qnk = 0;      // the quad's reward sums / list length / d_sen in steps
    for (int rep = 0, reps = REPS(11); rep < reps; ++rep) {
        FENCE();
        const int sub = lane & (LPA - 1);
        const float4 ha = hdr[ea];
        const float apr = ha.x, bpr = ha.y;
        const int ab0 = __float_as_int(ha.z), aca0 = __float_as_int(ha.w);
        const int ael = NPAD < 64 ? (ea & 63) / NPAD : 0;
        const LatEnv &La = P.lat[(blockIdx.x * EPB + ael) < P.n_env ? (blockIdx.x * EPB + ael) : P.n_env - 1];
        const float Rl = La.R;                                   // d_sen in lattice steps
        // the walk works in units of d_sen (coordinates scaled by 1 / R): u = da^2 + db^2 needs no further factor, and the
        // |v| threshold becomes the constant 0.05 / d_sen.  (1 / R to 1 ulp: inside the guard band's allowance for psi)
        const float inv_r = __builtin_amdgcn_rcpf(Rl);
        const float apr_s = apr * inv_r;
        const u64 *rma = lrm + ael * 64;
        const uint4 cq = reinterpret_cast<const uint4 *>(pcr)[ea];
        const int s0 = (int)__builtin_amdgcn_sad_u8(cq.x, 0u, 0u), s1 = (int)__builtin_amdgcn_sad_u8(cq.y, 0u, 0u);
        const int s2 = (int)__builtin_amdgcn_sad_u8(cq.z, 0u, 0u), s3 = (int)__builtin_amdgcn_sad_u8(cq.w, 0u, 0u);
        const int nk = s0 + s1 + s2 + s3;
        const int per = LIST_LEAN ? (int)((unsigned)(nk + LPA - 1) / (unsigned)LPA) : (nk + LPA - 1) / LPA;   // (nk >= 0: a shift)
        const int k0 = sub * per < nk ? sub * per : nk;
        const int k1 = k0 + per < nk ? k0 + per : nk;
        // the window row holding rank k0: the LAST row whose first rank is <= k0 (empty rows in front of it are skipped)
        int t, before;
        {
            const int c1 = s0, c2 = s0 + s1, c3 = c2 + s2;
            const int d = (k0 >= c1 ? 1 : 0) + (k0 >= c2 ? 1 : 0) + (k0 >= c3 ? 1 : 0);
            before = d == 0 ? 0 : (d == 1 ? c1 : (d == 2 ? c2 : c3));
            const unsigned wd = d == 0 ? cq.x : (d == 1 ? cq.y : (d == 2 ? cq.z : cq.w));
            const int e1 = before + (int)(wd & 255u), e2 = e1 + (int)((wd >> 8) & 255u), e3 = e2 + (int)((wd >> 16) & 255u);
            const int j = (k0 >= e1 ? 1 : 0) + (k0 >= e2 ? 1 : 0) + (k0 >= e3 ? 1 : 0);
            before = j == 0 ? before : (j == 1 ? e1 : (j == 2 ? e2 : e3));
            t = 4 * d + j;
        }
        const unsigned *srp = srow + t * AG + ea;                    // kept columns (17 bits) | first cell index of the row << 17
        const unsigned wd0 = *srp;
        unsigned kept = k0 < k1 ? (wd0 & 0x1FFFFu) : 0u;
        {   // drop the (k0 - before) lowest set bits: position of that set bit by a binary search on popcounts
            int pb = 0, left = k0 - before;
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) {
                const int c = __popc((kept >> pb) & ((1u << sh) - 1u));
                const bool go = left >= c;
                left -= go ? c : 0; pb += go ? sh : 0;
            }
            kept &= ~((1u << pb) - 1u);                              // pb <= 31: that set bit exists (k0 < k1)
        }
        int base = (int)(wd0 >> 17);
        // a lane with k0 < k1 only ever visits rows between two non-empty window rows -- rows of the lattice, 0 <= b < 64 --
        // so the walk needs no range check on the row; the first read of a lane without work is clamped
        const int bt0 = ab0 + t;
        const u64 *rmp = rma + (bt0 < 0 ? 0 : (bt0 > 63 ? 63 : bt0));
        unsigned relm = (unsigned)(*rmp >> aca0);
        float dbf = ((float)t - bpr) * inv_r, db2 = dbf * dbf;
        float n0 = 0.0f, n1 = 0.0f, dn = 0.0f;
        short *row = sidx + (size_t)ea * P.g_stride;
        const unsigned nm1 = (unsigned)(nk - 1);
        // rank(q) = round(q (n-1)/(G-1)) of list slot q (CPP:241-245), see the generic path for the integer form
        auto rank_of = [&](int q) -> int {
            if (P.cap_int) {
                const unsigned x = 2u * (unsigned)q * nm1 + (unsigned)(G - 1);
                const unsigned hq_ = __umulhi(x, P.cap_magic);
                return (int)((((x - hq_) >> 1) + hq_) >> P.cap_shift);
            }
            const double v = q * ((double)nm1 / (G - 1));
            return (int)(P.cap_even ? rint(v) : round(v));
        };
        auto walk_range = [&](auto capped) {
            constexpr bool CAP = decltype(capped)::value;
            int k = k0;
            // capped agent (n > G, rare): `slot` = number of selected ranks below k, `nxt` = the next selected rank
            int slot = k0, nxt = 0;
            if constexpr (CAP) {
                if (nk > G) {
                    // rank(q) < k  <=>  2 q (n-1) < (2k-1)(G-1) (integer form of the rounding, G-1 odd): a ceiling division
                    if (P.cap_int) slot = k0 > 0 ? (int)((unsigned)((2 * k0 - 1) * (G - 1) + 2 * (int)nm1 - 1) / (2u * nm1)) : 0;
                    else { slot = 0; while (slot < G && rank_of(slot) < k0) ++slot; }
                    slot = slot < G ? slot : G;
                    nxt = slot < G ? rank_of(slot) : 0x7FFFFFFF;
                }
            }
            while (__any(k < k1)) {
                if (k < k1) {
                    if (kept == 0) {                                 // next window row (more kept bits exist: k < k1 <= n)
                        srp += AG; ++rmp;
                        const unsigned wd = *srp;
                        kept = wd & 0x1FFFFu; base = (int)(wd >> 17);
                        relm = (unsigned)(*rmp >> aca0);
                        dbf += inv_r; db2 = dbf * dbf;
                    }
                    if (kept != 0) {
                        const int c = __ffs(kept) - 1;
                        kept &= kept - 1;
                        const int cell = base + __popc(relm & ((1u << c) - 1u));
                        bool take = true;
                        if constexpr (CAP) {
                            if (nk > G) {
                                take = k == nxt;
                                if (take) nxt = slot + 1 < G ? rank_of(slot + 1) : 0x7FFFFFFF;
                            }
                        }
                        if constexpr (CAP) { if (take) row[slot] = (short)cell; slot += take ? 1 : 0; }
                        else row[k] = (short)cell;                   // under the cap the slot of a cell is its rank
                        ++k;
                        const float da = fmaf((float)c, inv_r, -apr_s);
                        const float u = fmaf(da, da, db2);
                        float psi = psi5_u_f32(u);
                        if constexpr (CAP) psi = take ? psi : 0.0f;
                        n0 = fmaf(psi, da, n0); n1 = fmaf(psi, dbf, n1); dn += psi;
                    }
                }
            }
        };
        // (switched by LIST_LEAN alone, the loop a function outside the kernel: the other 150 kernels keep their code)
        if constexpr (LIST_LEAN) {
            if (__any(nk > G)) list_walk_lean<true, AG>(P, srow + t * AG + ea, rmp, aca0, k0, k1, k0 - before, nk, dbf, inv_r, apr_s, row, n0, n1, dn);
            else list_walk_lean<false, AG>(P, srow + t * AG + ea, rmp, aca0, k0, k1, k0 - before, nk, dbf, inv_r, apr_s, row, n0, n1, dn);
        } else {
            if (__any(nk > G)) walk_range(std::true_type{}); else walk_range(std::false_type{});
        }
        // the quad's partial sums -> every lane of the quad (two DPP exchanges)
        auto quad_sum = [](float v) -> float {
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
            return v;
        };
        auto lanes_sum = [&](float v) -> float {                     // ... and the second quad's sum into an 8-lane group's first lane
            v = quad_sum(v);
            if constexpr (LPA == 8) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x104, 0xF, 0xF, true));   // row_shl:4
            return v;
        };
        qn0 = lanes_sum(n0); qn1 = lanes_sum(n1); qdn = lanes_sum(dn); qnk = nk; qrl = Rl;
    }
    STAMP(19);
    EXIT_AT(9);
    // ---- (R) reward of the quad's agent (CPP:554-556), decided by the quad's first lane right here: everything it needs was
    // produced by this wave (the list, the sums) or long before (in-shape flag, collision flag).  The fp32 verdict only
    // DECIDES outside its guard band; an unsure agent is redone exactly by the whole wave.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // this wave's list rows: written above, read below
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
        const int nsl = qnk > G ? G : qnk;
        if constexpr (ROWS_LIVE) {
            // the longest list of each group of eight rows is its last agent's (ranking: key (length, lane)); taken here, on the
            // scalar side, while the lengths are in a register
            const int n0 = __builtin_amdgcn_readlane(nsl, 7 * LPA), n1 = __builtin_amdgcn_readlane(nsl, 15 * LPA);
            row_live = ((n0 + 15) >> 4) | (((n1 + 15) >> 4) << 4);
        }
        const bool in_a = (sncf[ea] >> 30) != 0;
        const int ael = NPAD < 64 ? (ea & 63) / NPAD : 0, ai = NPAD < 64 ? (ea & 63) % NPAD : ea;
        const int ae = blockIdx.x * EPB + ael;
        const bool lead = (lane & (LPA - 1)) == 0 && ae < P.n_env && ai < n_a;
        const bool has = lead && in_a && nsl > 0;
        const float thr = P.rew_thr_k;                               // 0.05 in units of d_sen (the walk's scale)
        const float idn = __builtin_amdgcn_rcpf(qdn);                // (1 ulp + two roundings: far inside the 4e-6 the band allows)
        const float v0f = qn0 * idn, v1f = qn1 * idn;
        const float vf = sqrtf(fmaf(v0f, v0f, v1f * v1f));
        bool uni = has && vf < thr;
        const float inv_rl = __builtin_amdgcn_rcpf(qrl);             // the band is kept in lattice steps on the host: scale it
        const bool uns = has && (P.force_exact || !(qdn > 1e-6f) || !(fabsf(vf - thr) > (P.rew_ga_lat * (float)nsl * idn + P.rew_gb_lat) * inv_rl * 1.0001f));
        u64 um = __ballot(uns);
        while (um != 0) {
            const int L = __ffsll((unsigned long long)um) - 1;
            um &= um - 1;
            const bool res = exact_uniform(__builtin_amdgcn_readlane(ea, L), __builtin_amdgcn_readlane(nsl, L), __builtin_amdgcn_readlane(ae, L));
            if (lane == L) uni = res;
        }
        if (lead) {
            const size_t oi = (size_t)ae * n_a + ai;
            if (reward != nullptr) __builtin_nontemporal_store((in_a && !(snei[ea * kNeiStride + kTopoMax] != 0) && uni) ? 1.0f : 0.0f, &reward[oi]);   // CPP:554-556
            if (done != nullptr) __builtin_nontemporal_store((uint8_t)0, &done[oi]);                                                                     // ENV:480-482
        }
    }
    STAMP(6);
    EXIT_AT(10);
    // Work that needs nothing from the list phase: the prior policy on split B, the observation heads on the two splits whose
    // lists were shortest (A and C); the split with the longest lists (D) goes straight to its rows.
    prior_policy();
    if (obs != nullptr) {
        if constexpr (TGT_LDS) head_blocks_tgt();
        else head_blocks(NW == 1);                   // (N > 64: dealt over all splits but B; the early A / C deal measured +15 % at N = 256)
        STAMP(9);
        EXIT_AT(11);
        if constexpr (ROWS_LIVE) {
            if (G == 80) sensed_rows_live(row_live);
            else sensed_rows(true, perm + (tid >> 6) * 64);
        } else sensed_rows(true, perm + (tid >> 6) * 64);
    }
    } else {
    // ---- occupied-cell filter, CPP:144-216: a sensed cell is occupied iff some nearby agent is within
    // r_avoid/2 of it; only agents inside the shape filter (CPP:150).  kept = in_shape ? sensed & ~occupied : sensed.
    // The words of the sensed set are filtered in place, dealt over the splits like the scan (each split filters the words
    // it scanned), and counted; the barrier that follows publishes the kept words and their counts to every split.
    {
        u64 nearby[NW];
#pragma unroll
        for (int q = 0; q < NW; ++q) nearby[q] = (NW > 1 && in_shape) ? snear[q * AG + at] : 0;
        for (int rep = 0, reps = REPS(4); rep < reps; ++rep)
        for (int w = 0; w < W; ++w) {
            if (!mine(w)) continue;
            FENCE();
            const unsigned word = sbits[w * AG + at];
            unsigned kw = word;
            if constexpr (NW == 1) {
                if (in_shape) kw = word & ~owords[w * AG + at];       // occupied bits came out of the scan
                if (rep == reps - 1) sbits[w * AG + at] = kw;
            } else if (in_shape) {
                unsigned it = word;
                while (it) {
                    int bb[4]; bool occ[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { bb[u] = it ? __ffs(it) - 1 : -1; it &= it - 1; }   // it - 1 of 0 is harmless: it stays 0
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int c = w * 32 + (bb[u] < 0 ? 0 : bb[u]);
                        occ[u] = false;
#pragma unroll
                        for (int q = 0; q < NW; ++q) occ[u] = occ[u] || ((cmask[(size_t)c * NW + q] & nearby[q]) != 0);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (bb[u] >= 0 && occ[u]) kw &= ~(1u << bb[u]);
                }
                if (rep == reps - 1) sbits[w * AG + at] = kw;
            }
            asm volatile("" :: "v"(kw));
            if (P.export_idx) obits[w * AG + at] = word & ~kw;
            pc[w * AG + at] = (unsigned char)__popc(kw);
        }
    }
    __syncthreads();
    STAMP(5);
    EXIT_AT(6);

    // ---- capped sensed list (CPP:236-271) into LDS, and the exploration reward's sums over it (CPP:494-551).
    // Each split emits the slots of its own words (rank = prefix of the kept-bit counts) and accumulates
    // partial sums; the sums are combined in split order below.
    int n_kept = 0;
    for (int w = 0; w < W; ++w) n_kept += pc[w * AG + at];
    n_sel = n_kept > G ? G : n_kept;
    // (1) which RANKS of the kept list survive the cap?  rank(s) = round(s * (n-1)/(G-1)), s = 0..G-1 (CPP:241-245),
    // evaluated in a uniform slot loop (split sx takes slots sx, sx+WPE, ...) and OR-ed into a per-lane bit set.
    // With G-1 odd the value s(n-1)/(G-1) is never within 1/(2(G-1)) of a half-integer, so the reference's fp64
    // round() equals the integer floor((2 s (n-1) + (G-1)) / (2 (G-1))) exactly; for even G-1 (ties possible) the
    // reference's fp64 expression is evaluated as is.
    unsigned *rsel = reinterpret_cast<unsigned *>(smem + P.off_cmask);      // [W+1][AG] (aliases cmask: consumed)
    for (int w = sx; w <= W; w += WPE) rsel[w * AG + at] = 0;
    __syncthreads();
    // The cap is rare (an agent deep inside a fine-celled shape): when no agent of this wave is capped -- the same
    // answer in all WPE splits, they hold the same agents -- ranks are slots and the rank-select bits are skipped.
    const bool any_sub = __any(n_kept > G) != 0;
    int *sub_base = reinterpret_cast<int *>(smem + P.off_partc);   // [WPE][AG] first slot of each split's rank range, capped agents only (part_c is consumed)
    // (for N <= 64 `any_sub` is the same in every wave of the workgroup, so the barriers it guards are uniform)
    if (any_sub)
    for (int rep = 0, reps = REPS(5); rep < reps; ++rep) {
        FENCE();
        const bool sub = n_kept > G;
        // lanes under the cap: rank = slot, i.e. bits [0, n_kept) -- whole words, dealt over the splits
        if (!sub)
            for (int w = sx; w * 32 < G; w += WPE) {
                const int left = n_kept - w * 32;
                if (left > 0) rsel[w * AG + at] = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
            }
        // capped lanes (rare, usually one or two per wave): wave-cooperative, lane = slot -- G/64 passes per capped agent
        // instead of every lane looping over its G slots; the capped agents are dealt over the splits
        u64 sm = __ballot(sub);
        int k = 0;
        while (sm != 0) {
            const int L = __ffsll((unsigned long long)sm) - 1;
            sm &= sm - 1;
            if ((k++ % WPE) != sx) continue;
            const unsigned nm1 = (unsigned)(__builtin_amdgcn_readlane(n_kept, L) - 1);
            const double step = (double)nm1 / (G - 1);
            unsigned *rl = rsel + (at & ~63) + L;                                  // agent thread of lane L in this wave
            const unsigned perL = (nm1 + 1 + WPE - 1) / WPE;                       // ranks per split in the emission below
            int below[WPE];                                                        // selected ranks below split s's first rank
#pragma unroll
            for (int sp_ = 0; sp_ < WPE; ++sp_) below[sp_] = 0;
            for (int q0 = 0; q0 < G; q0 += 64) {
                const int q = q0 + lane;
                unsigned r = 0xFFFFFFFFu;
                if (q < G) {
                    if (P.cap_int) {
                        const unsigned x = 2u * (unsigned)q * nm1 + (unsigned)(G - 1);
                        const unsigned hq = __umulhi(x, P.cap_magic);
                        r = (((x - hq) >> 1) + hq) >> P.cap_shift;                 // x / (2 (G-1)), Granlund-Montgomery
                    } else {
                        r = (unsigned)(int)(P.cap_even ? rint(q * step) : round(q * step));
                    }
                    atomicOr(&rl[(r >> 5) * AG], 1u << (r & 31));
                }
#pragma unroll
                for (int sp_ = 1; sp_ < WPE; ++sp_) below[sp_] += __popcll(__ballot(r < (unsigned)sp_ * perL));
            }
            if (lane == 0) {
#pragma unroll
                for (int sp_ = 1; sp_ < WPE; ++sp_) sub_base[sp_ * AG + (at & ~63) + L] = below[sp_];
            }
        }
    }
    if (NW > 1 || any_sub) __syncthreads();
    STAMP(18);
    EXIT_AT(7);
    // (2) emit: the kept list of an agent is cut into WPE contiguous RANK ranges, one per split.  Each lane walks its
    // own range bit by bit with a lane-private word pointer, so a wave's trip count is the longest range of any lane
    // (n_kept / WPE) -- not, as with words dealt over the splits, the sum over words of the fullest lane's count.
    int slot_lo = 0, slot_hi = 0;            // the slots this split emitted: its share of the reward sums below
    {
        short *row = sidx + (size_t)at * P.g_stride;
        for (int rep = 0, reps = REPS(11); rep < reps; ++rep) {
        FENCE();
        const int per = (n_kept + WPE - 1) / WPE;
        const int k0 = sx * per < n_kept ? sx * per : n_kept;
        const int k1 = k0 + per < n_kept ? k0 + per : n_kept;
        // the word holding rank k0 and the number of kept bits before k0 inside it
        int ww = 0, within = k0;
        {
            int prefix = 0;
            for (int w = 0; w < W; ++w) {                              // ww = number of words whose running count is <= k0
                prefix += pc[w * AG + at];
                const bool le = prefix <= k0;
                ww += le ? 1 : 0; within = le ? k0 - prefix : within;
            }
        }
        unsigned it = k0 < k1 ? sbits[ww * AG + at] : 0u;
        {   // drop the `within` lowest set bits: position of the within-th set bit by a binary search on popcounts
            int p = 0, left = within;
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) {
                const int c = __popc((it >> p) & ((1u << sh) - 1u));
                const bool go = left >= c;
                left -= go ? c : 0; p += go ? sh : 0;
            }
            it &= ~((1u << p) - 1u);                                   // p <= 31: the within-th set bit exists (k0 < k1)
        }
        // uncapped agent: rank = slot; capped: the rank-select pass counted the selected ranks below each split's range
        int slot = (n_kept > G && sx > 0) ? sub_base[sx * AG + at] : (n_kept > G ? 0 : k0);
        slot_lo = slot;
        // two instantiations of the walk: without a capped agent in the wave every kept bit is taken and no selection
        // word is carried
        auto walk_range = [&](auto capped) {
            constexpr bool CAP = decltype(capped)::value;
            int k = k0;
            unsigned rw = (CAP && k0 < k1) ? rsel[(k0 >> 5) * AG + at] : 0xFFFFFFFFu;      // selection bits of ranks 32 (k >> 5) ...
            while (__any(k < k1)) {
                if (k < k1) {
                    if (it == 0) { ++ww; it = sbits[ww * AG + at]; }         // next word (more kept bits exist: k < k1 <= n_kept)
                    if (it != 0) {
                        const int b = __ffs(it) - 1;
                        it &= it - 1;
                        const bool take = !CAP || ((rw >> (k & 31)) & 1u) != 0;
                        if (take) row[slot] = (short)(ww * 32 + b);
                        slot += take ? 1 : 0;
                        ++k;
                        if (CAP && (k & 31) == 0 && k < k1) rw = rsel[(k >> 5) * AG + at];
                    }
                }
            }
        };
        if (any_sub) walk_range(std::true_type{}); else walk_range(std::false_type{});
        slot_hi = slot;
        }
        for (int q = n_sel + sx; q < G; q += WPE) row[q] = -1;
    }
    STAMP(19);
    if (NW > 1 || any_sub) __syncthreads();      // the partial sums below overwrite the rank-select bits other splits may still read
    STAMP(20);
    EXIT_AT(8);
    // exploration-reward sums over the capped list (CPP:494-551), fp32 fast path: every split sums the slots it has just
    // emitted itself (its own LDS writes: no barrier in between), two per iteration in packed fp32.  The fp32 result
    // only DECIDES when |v| is outside a guard band around the 0.05 threshold; inside it the sums are redone in fp64 below.
    {
        const float inv_dsen2 = (float)(1.0 / (P.d_sen * P.d_sen));
        float num0 = 0.0f, num1 = 0.0f, den = 0.0f;
        const short *row = sidx + (size_t)at * P.g_stride;
        const int lim = in_shape ? slot_hi : slot_lo;
        for (int rep = 0, reps = REPS(6); rep < reps; ++rep) {
        FENCE();
        f2v n0v = {0.0f, 0.0f}, n1v = {0.0f, 0.0f}, dnv = {0.0f, 0.0f};
        const f2v pxx2 = {pxf, pxf}, pyy2 = {pyf, pyf}, inv2 = {inv_dsen2, inv_dsen2};
        for (int q = slot_lo; __any(q < lim); q += 2) {
            const bool va = q < lim, vb = q + 1 < lim;
            const int ca = va ? row[q] : 0, cb = vb ? row[q + 1] : 0;         // cell 0 stands in for an empty slot (weight zeroed)
            f2v gx, gy;
            gx = f2v{cq_e[(ca >> 1) * 4 + (ca & 1)], cq_e[(cb >> 1) * 4 + (cb & 1)]};
            gy = f2v{cq_e[(ca >> 1) * 4 + 2 + (ca & 1)], cq_e[(cb >> 1) * 4 + 2 + (cb & 1)]};
            const f2v x = gx - pxx2, y = gy - pyy2;
            const f2v u = __builtin_elementwise_fma(x, x, y * y) * inv2;
            f2v c = {7.969553699e-04f, 7.969553699e-04f};                      // psi_u_f32, both slots at once
            c = __builtin_elementwise_fma(c, u, f2v{-1.267949212e-02f, -1.267949212e-02f});
            c = __builtin_elementwise_fma(c, u, f2v{1.175149009e-01f, 1.175149009e-01f});
            c = __builtin_elementwise_fma(c, u, f2v{-6.675792336e-01f, -6.675792336e-01f});
            c = __builtin_elementwise_fma(c, u, f2v{2.029347420e+00f, 2.029347420e+00f});
            c = __builtin_elementwise_fma(c, u, f2v{-2.467400551e+00f, -2.467400551e+00f});
            c = __builtin_elementwise_fma(c, u, f2v{1.0f, 1.0f});
            const f2v psi = {va ? c.x : 0.0f, vb ? c.y : 0.0f};
            n0v = __builtin_elementwise_fma(psi, x, n0v); n1v = __builtin_elementwise_fma(psi, y, n1v); dnv = dnv + psi;
        }
        num0 = n0v.x + n0v.y; num1 = n1v.x + n1v.y; den = dnv.x + dnv.y;
        }
        rsum[(sx * 3 + 0) * AG + at] = num0; rsum[(sx * 3 + 1) * AG + at] = num1; rsum[(sx * 3 + 2) * AG + at] = den;
    }
    STAMP(21);
    __syncthreads();
    STAMP(6);
    EXIT_AT(9);

    if (sx == 0) {
        float n0 = 0.0f, n1 = 0.0f, dn = 0.0f;
#pragma unroll
        for (int s = 0; s < WPE; ++s) {
            n0 += rsum[(s * 3 + 0) * AG + at]; n1 += rsum[(s * 3 + 1) * AG + at]; dn += rsum[(s * 3 + 2) * AG + at];
        }
        const bool has = in_shape && n_sel > 0;
        const float v0f = n0 / dn, v1f = n1 / dn;
        const float vf = sqrtf(fmaf(v0f, v0f, v1f * v1f));
        uniform = has && vf < 0.05f;
        unsure = has && (P.force_exact || !(dn > 1e-6f) || !(fabsf(vf - 0.05f) > P.rew_ga * (float)n_sel / dn + P.rew_gb));
    }
    }

    if constexpr (!LAT) {
        // generic path: split A combines the splits' fp32 sums (above) and stores the reward
        if (sx == 0) {
            u64 um = __ballot(unsure);
            while (um != 0) {
                const int L = __ffsll((unsigned long long)um) - 1;               // agent thread, wave-uniform
                um &= um - 1;
                const bool res = exact_uniform((at & ~63) + L, __builtin_amdgcn_readlane(n_sel, L), blockIdx.x * EPB + (NPAD < 64 ? L / NPAD : 0));
                if (lane == L) uniform = res;
            }
            if (act) {
                if (reward != nullptr) __builtin_nontemporal_store((in_shape && !(snei[at * kNeiStride + kTopoMax] != 0) && uniform) ? 1.0f : 0.0f, &reward[(size_t)e * n_a + i]);   // CPP:554-556
                if (done != nullptr) __builtin_nontemporal_store((uint8_t)0, &done[(size_t)e * n_a + i]);                                                         // ENV:480-482
            }
        }
    }
    if (P.export_idx) {
        if constexpr (LAT) __syncthreads();          // export launches only (workgroup-uniform): every wave's lists are complete
        if (sx == 0) {
        if (P.export_idx && act) {
            const short *row = sidx + (size_t)at * P.g_stride;
            int *es_ = P.exp_sensed + ((size_t)e * n_a + i) * G;
            for (int q = 0; q < G; ++q) es_[q] = row[q];
            // occupied list with its own cap, CPP:217-233.  NWD words of occupied bits in ascending cell order: the target-cell
            // words of the generic scan, or the window rows of the lattice path (row-major = ascending cell index)
            const int NWD = LAT ? P.lat_nrs : W;
            const unsigned *ob = LAT ? orow : obits;
            int ob0 = 0, oca0 = 0;
            if constexpr (LAT) { const float4 hq = hdr[at]; ob0 = __float_as_int(hq.z); oca0 = __float_as_int(hq.w); }
            int n_occ = 0;
            for (int w = 0; w < NWD; ++w) n_occ += __popc(ob[w * AG + at]);
            const int O = P.occ_max;
            int *eo = P.exp_occ + ((size_t)e * n_a + i) * O;
            const bool osub = n_occ > O;
            const double ostep = osub ? (double)(n_occ - 1) / (O - 1) : 0.0;
            int os = 0, ok = 0, otarget = 0;
            for (int w = 0; w < NWD; ++w) {
                unsigned it = ob[w * AG + at];
                int cbase = w * 32; unsigned relm = 0xFFFFFFFFu;           // generic: cell = 32 w + bit
                if constexpr (LAT) {
                    const int bq = ob0 + w < 0 ? 0 : (ob0 + w > 63 ? 63 : ob0 + w);
                    const u64 rowm = lrm[el * 64 + bq];
                    cbase = lrs[el * 64 + bq] + __popcll(rowm & ((1ull << oca0) - 1ull)); relm = (unsigned)(rowm >> oca0);
                }
                while (it) {
                    const int b = __ffs(it) - 1;
                    it &= it - 1;
                    const bool sel = osub ? (ok == otarget) : true;
                    if (sel && os < O) { eo[os++] = cbase + __popc(relm & ((1u << b) - 1u)); if (osub) otarget = (int)round(os * ostep); }
                    ++ok;
                }
            }
            for (; os < O; ++os) eo[os] = -1;
        }
        }
    }
    STAMP(22);
    if constexpr (!LAT) {
        EXIT_AT(10);
        prior_policy();
        if (obs != nullptr) {
            head_blocks(false);
            STAMP(9);
            EXIT_AT(11);
            sensed_rows(false, nullptr);
        }
    }
    STAMP(7);
#ifdef SWARM_STAMPS
    if (P.stamps != nullptr && lane == 0) P.stamps[((size_t)blockIdx.x * (T / 64) + (tid >> 6)) * 24 + 23] = sx;   // slot 23 = the wave's split (role)
#endif
}

#undef LO

}  // namespace

#if SWARM_UNIT_KERNELS
// ---- the kernel part: the instantiations of one agent count (a kernel unit) or of all six (the whole file), with their
// launch -- hipFuncSetAttribute wants the kernel's address, which only the unit that instantiates the kernel has

namespace {

template <int NPAD, typename OT, bool DO_STEP, bool LAT, bool HALF, bool FILT = false>
int launch_t(swarm_env *h, const Launch &l, const Pass &ps)
{
    constexpr int T = Geo<NPAD, HALF>::T, EPB = Geo<NPAD, HALF>::EPB;
    auto kern = k_env<NPAD, OT, DO_STEP, LAT, HALF, FILT>;
    const KP &kp = *l.kp;
    int smem = !LAT ? kp.smem_generic : (kp.export_idx ? kp.smem_lat_export : kp.smem_lat);
#ifdef SWARM_EXTRA_SMEM
    smem += SWARM_EXTRA_SMEM;                            // occupancy experiments only
#endif
    int &attr = h->attr_smem[attr_slot(sizeof(OT), DO_STEP, LAT, HALF, FILT)];   // raise the dynamic-LDS cap once per instantiation
    if (attr < smem) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr = smem;
    }
    const int grid = (h->cfg.n_env + EPB - 1) / EPB;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(T), smem, l.st, kp, ps.action, ps.act_mode,
                       static_cast<OT *>(ps.obs), ps.reward, ps.done, static_cast<OT *>(ps.a_prior));
    HIP_TRY(h, hipGetLastError());
    return SWARM_OK;
}

// The instantiation of one agent count that l and ps ask for.  The kernels stand in the code object in the order of
// instantiation: steps before observation passes (launch_npad), then with_obs_type's order, then the order below.
template <int NPAD, bool DO_STEP>
int launch_n(swarm_env *h, const Launch &l, const Pass &ps)
{
    return with_obs_type(h->cfg.obs_dtype, [&](auto t) {
        typedef typename decltype(t)::type OT;
        const bool lat = l.kp->lattice != 0;
        if constexpr (NPAD < 64) {
            if (lat && l.half) return launch_t<NPAD, OT, DO_STEP, true, true>(h, l, ps);
        }
        if (l.kp->path_filter != 0) {              // a launch of a mixed batch: 1 = its lattice launch, 2 = its generic launch
            if (l.kp->path_filter != (lat ? 1 : 2) || l.half) return fail(h, SWARM_ERR_INVALID, "env_launch: path_filter does not match the launch");
            return lat ? launch_t<NPAD, OT, DO_STEP, true, false, true>(h, l, ps) : launch_t<NPAD, OT, DO_STEP, false, false, true>(h, l, ps);
        }
        return lat ? launch_t<NPAD, OT, DO_STEP, true, false>(h, l, ps) : launch_t<NPAD, OT, DO_STEP, false, false>(h, l, ps);
    });
}

}  // namespace

namespace swarm_internal {

template <int NPAD>
int launch_npad(swarm_env *h, const Launch &l, const Pass &ps)
{
    return ps.do_step ? launch_n<NPAD, true>(h, l, ps) : launch_n<NPAD, false>(h, l, ps);
}

#ifdef SWARM_ENV_UNIT
template int launch_npad<SWARM_ENV_UNIT>(swarm_env *, const Launch &, const Pass &);
#else
template int launch_npad<8>(swarm_env *, const Launch &, const Pass &);
template int launch_npad<16>(swarm_env *, const Launch &, const Pass &);
template int launch_npad<32>(swarm_env *, const Launch &, const Pass &);
template int launch_npad<64>(swarm_env *, const Launch &, const Pass &);
template int launch_npad<128>(swarm_env *, const Launch &, const Pass &);
template int launch_npad<256>(swarm_env *, const Launch &, const Pass &);
#endif

}  // namespace swarm_internal

#endif  // SWARM_UNIT_KERNELS

#if SWARM_UNIT_HOST
// ---- the host part: the LDS layout, the geometries, the choice of the launch, the diagnostic entry points.  No kernel is
// instantiated here.

namespace {

template <int NPAD, bool HALF>
void layout_t(KP &k)
{
    typedef Geo<NPAD, HALF> G_;
    constexpr int AG = G_::AG, EPB = G_::EPB, NW = G_::NW, WPE = G_::WPE, T = G_::T;
    k.ngw = (k.ng_max + 31) / 32;
    int half = (k.g_max + 1) / 2;
    if ((half & 1) == 0) ++half;              // odd dword stride: lane-per-row int16 writes spread over banks
    k.g_stride = 2 * half;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 15) & ~size_t(15); return (int)o; };
    auto max2 = [](size_t a, size_t b) { return a > b ? a : b; };
    const size_t pm_bytes = (size_t)(NW == 1 ? WPE * 4 : 5) * NW * AG * 8;   // partial pair masks (per-split copies for N <= 64, one accumulator set above)
    k.off_cxy = 0;                             // fp64 cells are no longer staged in LDS (cxy_stride, off_rres: dead too, left zero)
    k.off_sp = take((size_t)4 * AG * 8);
    k.cxq_stride = k.ngw * 64 + 4;             // floats: 2 per cell, +1 pair-of-pairs of padding
    if (k.lattice) {
        // row-space lattice path: no per-cell bit sets at all.  The map is LatMap's.  Geometries with G_::CT_MAP address every
        // region through the same compile-time constants and read none of the run-time offsets but off_orow; the others read the
        // offsets below, which are the same map's
        typedef LatMap<NPAD, HALF> LM;
        k.smem_lat = LM::total(k.g_stride);              // lattice mode, no export
        k.off_orow = LM::orow_off(k.g_stride);           // only launches that export the index scratch use it
        k.smem_lat_export = LM::total_export(k.g_stride);
        k.off_sp = LM::sp; k.off_hdr = LM::hdr; k.off_srow = LM::srow; k.off_pcr = LM::pcr; k.off_sidx = LM::sidx;
        k.off_partc = LM::partc; k.off_partd = LM::partd; k.off_lat = LM::lat; k.off_cov = LM::cov; k.off_flag = LM::flag;
        k.off_snei = LM::snei; k.off_sncf = LM::sncf; k.off_snear = LM::snear; k.off_perm = LM::perm; k.off_rres = 0;
        k.off_cmask = k.off_sbits = k.off_obits = k.off_pc = k.off_cxyf = 0;     // generic scan only
        k.smem_generic = 0;
        return;
    }
    k.off_cmask = take(max2(max2((size_t)k.ngw * 32 * NW * 8, (size_t)WPE * 3 * AG * 4 + (NW > 1 ? NW * 1536 : 0)), (size_t)(k.ngw + 1) * AG * 4));   // cmask | rsel | rsum
    k.off_sbits = take((size_t)(k.ngw + 1) * AG * 4);
    k.off_sidx = take(max2(max2((size_t)AG * k.g_stride * 2, pm_bytes), (size_t)14 * AG * 8));
    k.off_partc = take((size_t)WPE * AG * 4);
    // lat, cov, flag: unread by the generic kernel (flag is cleared in its prologue, by a store nobody reads).  They stay: the
    // launch's LDS bytes decide occupancy, and a change of those wants an A/B run on hardware
    k.off_lat = take((size_t)EPB * 64 * (8 + 2));
    k.off_cov = take((size_t)EPB * (k.ngw + 1) * 4);
    k.off_flag = take((size_t)AG * 4);
    k.off_snei = take((size_t)AG * kNeiStride * 2);
    k.off_sncf = take((size_t)AG * 4);
    k.off_snear = take((size_t)NW * AG * 8);
    k.off_pc = take((size_t)k.ngw * AG);
    k.off_obits = take((size_t)k.ngw * AG * 4);
    k.off_cxyf = take((size_t)EPB * k.cxq_stride * 4);   // fp32 cell copy of the generic scan
    k.smem_generic = (int)off;
    k.smem_lat = k.smem_lat_export = 0;
    k.off_hdr = k.off_srow = k.off_pcr = k.off_perm = k.off_rres = k.off_orow = k.off_partd = 0;
}

// f(Geo<NPAD, HALF>{}) for the geometry of npad / half: the list of geometries, in one place
template <typename F>
void for_geometry(int npad, bool half, F &&f)
{
    switch (npad) {
    case 8: if (half) f(Geo<8, true>{}); else f(Geo<8, false>{}); break;
    case 16: if (half) f(Geo<16, true>{}); else f(Geo<16, false>{}); break;
    case 32: if (half) f(Geo<32, true>{}); else f(Geo<32, false>{}); break;
    case 64: f(Geo<64, false>{}); break;
    case 128: f(Geo<128, false>{}); break;
    default: f(Geo<256, false>{}); break;
    }
}

// one launch of the step kernel: the instantiation of the handle's agent count and obs dtype that l asks for
int launch_one(swarm_env *h, const Launch &l, const Pass &ps)
{
    switch (h->npad) {
    case 8: return launch_npad<8>(h, l, ps);
    case 16: return launch_npad<16>(h, l, ps);
    case 32: return launch_npad<32>(h, l, ps);
    case 64: return launch_npad<64>(h, l, ps);
    case 128: return launch_npad<128>(h, l, ps);
    case 256: return launch_npad<256>(h, l, ps);
    }
    return fail(h, SWARM_ERR_INVALID, "unsupported agent count");
}

}  // namespace

namespace swarm_internal {

void env_layout(KP &k, int npad, bool half)
{
    for_geometry(npad, half, [&](auto g) { layout_t<decltype(g)::NPAD_, decltype(g)::HALF_>(k); });
}

GeoInfo env_geometry(int npad, bool half)
{
    GeoInfo r = {};
    for_geometry(npad, half, [&](auto g) { r = GeoInfo{decltype(g)::EPB, decltype(g)::T}; });
    return r;
}

const KP &launch_kp(const swarm_env *h, const Pass &ps, int filter, KP &tmp)
{
    if (filter == 0 && !ps.export_small && !ps.export_lists && !ps.cap_even && !ps.stamps) return h->kp;
    tmp = h->kp;
    tmp.export_small = ps.export_small; tmp.cap_even = ps.cap_even; tmp.stamps = ps.stamps;
    if (ps.export_lists) { tmp.export_idx = 1; tmp.exp_sensed = h->d_exp_sensed.get(); tmp.exp_occ = h->d_exp_occ.get(); }
    tmp.path_filter = filter;
    if (filter == 2) { tmp.lattice = 0; env_layout(tmp, h->npad, false); }
    return tmp;
}

int env_launch(swarm_env *h, const Pass &ps)
{
    KP tmp, tmp_gen;
    if (h->path_mode != PATH_MIXED)          // one kernel for the whole batch, as the handle's KP describes it
        return launch_one(h, Launch{&launch_kp(h, ps, 0, tmp), h->stream, h->half}, ps);
    // A mixed batch: the generic kernel steps the workgroups that hold an env without a lattice record, the lattice kernel the
    // others; both over the full geometry, so that they agree on which envs a workgroup holds, and each returns at once from
    // the other's workgroups (KP::path_filter).  The generic launch's KP is the lattice launch's (the pass's switches and
    // all) with the generic LDS layout.  The launches touch disjoint envs, so the generic one runs beside the lattice one on the
    // handle's auxiliary stream, forked from and joined to the handle's stream by events -- no host synchronisation;
    // debug_flags bit 4: one after the other on the handle's stream.
    const KP *lat = &launch_kp(h, ps, 1, tmp), *gen = &launch_kp(h, ps, 2, tmp_gen);
    if (h->cfg.debug_flags & 16) {
        const int rc = launch_one(h, Launch{gen, h->stream, false}, ps);
        if (rc != SWARM_OK) return rc;
        return launch_one(h, Launch{lat, h->stream, false}, ps);
    }
    if (!h->aux_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
    if (!h->ev_fork) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    if (!h->ev_join) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
    // from here the aux stream may hold work: nothing returns before the streams are joined again
    const int rc_gen = launch_one(h, Launch{gen, h->aux_stream, false}, ps);
    hipError_t e_join = hipEventRecord(h->ev_join, h->aux_stream);
    const int rc_lat = launch_one(h, Launch{lat, h->stream, false}, ps);
    if (e_join == hipSuccess) e_join = hipStreamWaitEvent(h->stream, h->ev_join, 0);
    if (e_join != hipSuccess) {                  // no event to wait on: the host waits for the generic launch instead (under a
                                                 // graph capture that wait fails too; the call is failing already and says so)
        (void)hipStreamSynchronize(h->aux_stream);
        if (rc_gen == SWARM_OK && rc_lat == SWARM_OK) HIP_TRY_AS(h, "joining the generic launch of a mixed batch", e_join);
    }
    return rc_gen != SWARM_OK ? rc_gen : rc_lat;
}

}  // namespace swarm_internal

extern "C" {

// Diagnostic, host only (no device, no handle): the LDS map of the lattice launches of one instantiation, for the CPU test
// that holds it in place.  out[0..1] = smem_lat / smem_lat_export as env_layout() hands them to the launches, out[2] = g_stride,
// out[3] = off_orow, out[4..15] = the kernel's compile-time offsets of sp, hdr, srow, pcr, partc, partd, lat, cov, flag, snei,
// sncf, sidx, out[16..27] = the same regions' run-time offsets in KP (read by the geometries without Geo::CT_MAP),
// out[28] = Geo::CT_MAP.  Returns 0, or -1 for a geometry that has no instantiation.
int swarm_debug_lds_map(int npad, int half, int g_max, int *out)
{
    if (!out || g_max < 1 || (half && npad >= 64)) return -1;
    if (npad != 8 && npad != 16 && npad != 32 && npad != 64 && npad != 128 && npad != 256) return -1;
    KP k;
    std::memset(&k, 0, sizeof(k));
    k.g_max = g_max; k.ng_max = 32; k.lattice = 1;
    env_layout(k, npad, half != 0);
    out[0] = k.smem_lat; out[1] = k.smem_lat_export; out[2] = k.g_stride; out[3] = k.off_orow;
    for_geometry(npad, half != 0, [&](auto g) {
        typedef LatMap<decltype(g)::NPAD_, decltype(g)::HALF_> LM;
        const int o[12] = {LM::sp, LM::hdr, LM::srow, LM::pcr, LM::partc, LM::partd, LM::lat, LM::cov, LM::flag, LM::snei, LM::sncf, LM::sidx};
        for (int q = 0; q < 12; ++q) out[4 + q] = o[q];
        out[28] = decltype(g)::CT_MAP ? 1 : 0;
    });
    const int r[12] = {k.off_sp, k.off_hdr, k.off_srow, k.off_pcr, k.off_partc, k.off_partd, k.off_lat, k.off_cov, k.off_flag, k.off_snei, k.off_sncf, k.off_sidx};
    for (int q = 0; q < 12; ++q) out[16 + q] = r[q];
    return 0;
}

#ifdef SWARM_STAMPS
// Diagnostic build only: run one step with per-wave phase clocks; out[grid][waves per workgroup][24] (host), returns grid size.
int swarm_debug_stamps(swarm_env_t *h, const void *action, int action_dtype, void *obs, float *reward, uint8_t *done,
                       void *a_prior, long long *out, int max_blocks)
{
    if (!h || !out) return -1;
    DeviceGuard g(h->device);
    const GeoInfo geo = env_geometry(h->npad, h->half);
    const int grid = (h->cfg.n_env + geo.envs - 1) / geo.envs;
    const int wpb = geo.threads / 64;                  // waves per workgroup
    if (grid > max_blocks) return -1;
    DevBuf<long long> d;
    if (d.alloc((size_t)grid * wpb * 24) != hipSuccess) return -1;
    (void)hipMemset(d.get(), 0, (size_t)grid * wpb * 24 * sizeof(long long));
    Pass ps = {true, action, action_dtype == SWARM_F64 ? ACT_F64 : 0, obs, reward, done, a_prior};
    ps.stamps = d.get();
    int rc = env_launch(h, ps);
    if (rc == SWARM_OK && hipMemcpy(out, d.get(), (size_t)grid * wpb * 24 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    return rc == SWARM_OK ? grid : -1;
}
#endif

}  // extern "C"

#endif  // SWARM_UNIT_HOST
