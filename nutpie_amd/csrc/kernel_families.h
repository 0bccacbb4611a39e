// kernel_families.h — the families of k_advance instantiations, in one table.
//
// Everything that has to agree on "which k_advance<...> runs this job" reads it from here: the geometry choice of the host
// (host.hip: choose_geometry), the launchers (kernels.hip: launch_family), the kernel's own occupancy attribute and the lean
// kernels' LDS split (Machine::LR_FREE).  Plain constexpr C++: host and device passes include it alike.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

// ---- waves per SIMD the kernels are compiled for (overridable with -D: measurements) ----------------------------------------
// one wave per chain: up to this many chunks per lane the kernel is built for two waves per SIMD (256 registers each).
// Not the kernel of a runtime-compiled density: its workgroup's LDS (four chains' scratch + the model's shared block) leaves one
// workgroup per CU anyway, and the density wants the registers — radon, 512 / 2048 chains, same box: 56.6 -> 62.1 / 96.2 -> 107.7 M
// leapfrogs/s for the traced torch density, 50.3 -> 51.5 / 90.6 -> 93.7 for the one written as expressions (profiles/r5_jit_occupancy.txt);
// a small density stays below 256 registers by itself.
#ifndef NPHIP_W1_OCC2_MAX
#ifdef NPHIP_JIT_DENSITY
#define NPHIP_W1_OCC2_MAX 0
#else
#define NPHIP_W1_OCC2_MAX 3
#endif
#endif
// register kernels with several waves per chain: up to this many chunks per wave run two waves per SIMD (256 registers each)
#ifndef NPHIP_RW_OCC2_MAX
#define NPHIP_RW_OCC2_MAX 4
#endif
#ifndef NPHIP_CB_OCC
// waves per SIMD the launch-per-evaluation (callback) kernels are compiled for.  Two: 256 registers per lane, (almost) nothing
// spilled.  Measured at four waves per SIMD (128 registers, every chain of a 1024-chain batch x 4 waves on the device at once):
// 82 spilled VGPRs, eleven of them stored by every wave of every launch — 23 MB of scratch traffic per launch in a kernel that
// is bound by its memory traffic — 38.4 us per launch against 33.5 (profiles/r4_callback_kernels.txt)
#define NPHIP_CB_OCC(W) 2
#endif
#ifndef NPHIP_LEAN_OCC
// waves per SIMD of the lean kernels: 8 waves = one chain per CU at 256 VGPRs per wave (4 waves: 512 = VGPRs + AGPRs)
#define NPHIP_LEAN_OCC(W) ((W) <= 4 ? 1 : ((W) <= 8 ? 2 : 4))
#endif

namespace nphip {

// (the names -DNPHIP_ONLY_FAMILY= takes)
enum class Family : int { w1, w1_wide, w1_lr, ring, ring_lr, lean, memory, remote, dense_resident };
inline constexpr const char* kFamilyNames[] = {"w1", "w1_wide", "w1_lr", "ring", "ring_lr", "lean", "memory", "remote", "dense_resident"};

enum class DynLds : int {
    none,
    sigma2,               // sigma^2 of the chain [ld]
    sigma2_and_summary,   // ... and as much of one (p, rho) summary as fits beside it (lean_free_chunks)
    sigma2_if_staged      // sigma^2 at 8 waves per chain and more, when the host asked for it (Args::sig_lds)
};

struct KernelFamily {
    Family family;
    bool fused, lean, remote, lr, wide, denseg;   // the flags of k_advance<FUSED, W, NV, LEAN, REMOTE, LR, WIDE, DENSEG>
    int waves;            // waves per chain it is built for, or-ed together (they are powers of two)
    int nv_lo, nv_hi;     // chunks of 128 elements per wave, inclusive (<= 0: the memory-resident forms)
    int part;             // its translation unit (Makefile: -DNPHIP_PART)
    DynLds dyn;
};

//                                               family                 fused  lean   remote lr     wide   denseg waves               nv      part  dynamic LDS
// register-resident, one wave per chain (D <= 1024): four chains per workgroup, one instantiation per exact chunk count
inline constexpr KernelFamily kW1One         = {Family::w1,             true,  false, false, false, false, false, 1,                  1, 1,   0,    DynLds::none};
// ... 2 .. 8 chunks per lane: a translation unit of its own, compiled without inter-procedural register allocation
inline constexpr KernelFamily kW1            = {Family::w1,             true,  false, false, false, false, false, 1,                  2, 8,   12,   DynLds::none};
// ... without the two-waves-per-SIMD register cap: what a job of at most kWideMaxChains chains is launched with
inline constexpr KernelFamily kW1Wide        = {Family::w1_wide,        true,  false, false, false, true,  false, 1,                  2, 3,   12,   DynLds::none};
// ... under the low-rank metric (settings.low_rank_metric; Machine<..., LR>)
inline constexpr KernelFamily kW1Lr          = {Family::w1_lr,          true,  false, false, true,  false, false, 1,                  1, 8,   8,    DynLds::none};
// register-resident with the LDS ring, several waves per chain (1024 < D <= 4096, or fewer chains than SIMDs): one workgroup = one chain
inline constexpr KernelFamily kRing          = {Family::ring,           true,  false, false, false, false, false, 2 | 4,              1, 8,   3,    DynLds::none};
// ... under the low-rank metric: the geometries the default waves per chain give (1024 < D <= 2048: two waves, 2048 < D <= 4096: four)
inline constexpr KernelFamily kRingLr        = {Family::ring_lr,        true,  false, false, true,  false, false, 2 | 4,              5, 8,   9,    DynLds::none};
// lean register-resident, 4 waves per chain (4096 < D <= 12288): state spread over VGPRs + AGPRs (one wave per SIMD).  21 .. 24 chunks
// per wave (10 240 < D <= 12 288, round 6): the state no longer fits the 512 registers of a lane — 16 per chunk beside a working set of
// ~130 — and the build spills (22 chunks: 216 bytes of scratch per lane, 24: 456); still 1.6 x / 1.3 x the memory-resident kernels that
// ran these rows before (D = 11 264: 8.6 against 5.4 M leapfrogs/s, D = 12 000: 6.5 against 5.0; profiles/r6_lean4_beyond_20_chunks.txt)
inline constexpr KernelFamily kLean4         = {Family::lean,           true,  true,  false, false, false, false, 4,                  9, 24,  1,    DynLds::sigma2_and_summary};
// lean register-resident, 8 waves per chain (on request: waves_per_chain = 8)
inline constexpr KernelFamily kLean8         = {Family::lean,           true,  true,  false, false, false, false, 8,                  1, 10,  2,    DynLds::sigma2};
// memory-resident: fused models of any D and W (D > 12 288, no_register_kernel, NV = -1: the low-rank metric) and, with FUSED = false, the
// two-phase callback kernels
inline constexpr KernelFamily kMemory        = {Family::memory,         true,  false, false, false, false, false, 1 | 2 | 4 | 8 | 16, -1, 0,  4,    DynLds::sigma2_if_staged};
// ... with the cursor's (sigma^2, grad, p, rho) of -NV chunks cached in VGPRs between leaves.  Measured with more waves per chain
// (D > 1024) the cache costs occupancy or spills and does not pay; W == 1 only.
inline constexpr KernelFamily kMemoryCached  = {Family::memory,         true,  false, false, false, false, false, 1,                  -8, -8, 4,    DynLds::none};
// resident launch of a host-callback job: the register-resident leaf with the evaluation as a rendezvous with the host
inline constexpr KernelFamily kRemoteW1      = {Family::remote,         false, false, true,  false, false, false, 1,                  1, 8,   5,    DynLds::none};
inline constexpr KernelFamily kRemoteWn      = {Family::remote,         false, false, true,  false, false, false, 2 | 4,              1, 8,   6,    DynLds::none};
// resident form of the dense-precision Gaussian (compiled without inter-procedural register allocation)
inline constexpr KernelFamily kDenseResident = {Family::dense_resident, false, false, true,  false, false, true,  1,                  1, 8,   11,   DynLds::none};

inline constexpr KernelFamily kFamilies[] = {kW1One, kW1, kW1Wide, kW1Lr, kRing, kRingLr, kLean4, kLean8, kMemory, kMemoryCached, kRemoteW1, kRemoteWn, kDenseResident};

// Chunk counts per lane at which the one-wave fused kernels with the diagonal metric (kW1, kW1Wide) take the two leaves of a level-0 pair in one
// trip (kernels.hip: Machine::pair_first): bit NV of the mask.  Measured per chunk count against the single leaf: profiles/leaf_pairs_d1000.txt.
#ifndef NPHIP_LEAF_PAIRS_NV_MASK
#define NPHIP_LEAF_PAIRS_NV_MASK 0x1FC
#endif
constexpr bool leaf_pairs(int W, int NV) { return W == 1 && NV >= 2 && NV <= 8 && ((NPHIP_LEAF_PAIRS_NV_MASK >> NV) & 1) != 0; }

inline constexpr int kWideMaxChains = 1024;   // k_advance<..., WIDE>: a job that brings at most one wave per SIMD
// waves per chain of the memory-resident kernels beyond the register families; measured at D = 10 000: W = 8 (5.5 M leapfrogs/s) beats 4 (5.0) and 16 (3.6)
inline constexpr int kMemoryWaves = 8;
inline constexpr int kMaxWaves = 16;

constexpr bool has(const KernelFamily& f, int W, int64_t nv) { return W > 0 && (f.waves & W) == W && (W & (W - 1)) == 0 && nv >= f.nv_lo && nv <= f.nv_hi; }
constexpr int chains_per_group(int W) { return W == 1 ? 4 : 1; }               // one wave per chain: a workgroup holds four chains
constexpr int group_threads(int W) { return 64 * W * chains_per_group(W); }

// Lean kernels, 4 waves per chain: chunks per wave of LDS left beside sigma^2 (the kernel's static LDS grows with the edge buffer: 8.1 KB
// at 20 chunks).  Machine::LR_FREE and the host's dynamic-LDS size are both this.
inline constexpr int kLdsBytes = 160 * 1024, kChunkBytes = 128 * 8;
constexpr int lean_free_chunks(int W, int nv) { return W == 4 ? (kLdsBytes - (nv > 20 ? 12288 : 8192) - nv * W * kChunkBytes) / (W * kChunkBytes) : 0; }

constexpr size_t dyn_lds_bytes(const KernelFamily& f, int W, int nv, int64_t ld, bool sig_lds) {
    const size_t sigma2 = (size_t)ld * 8;
    const int free_chunks = lean_free_chunks(W, nv), summary = free_chunks < 0 ? 0 : (free_chunks < 2 * nv ? free_chunks : 2 * nv);
    return f.dyn == DynLds::sigma2 ? sigma2
         : f.dyn == DynLds::sigma2_and_summary ? sigma2 + (size_t)summary * (size_t)(W * kChunkBytes)
         : (f.dyn == DynLds::sigma2_if_staged && W >= 8 && sig_lds) ? sigma2 : 0;
}

// the two bounds of k_advance's amdgpu_waves_per_eu
constexpr bool two_waves_per_simd(int W, int NV, bool LR, bool WIDE) { return NV > 0 && !LR && !WIDE && NV <= (W == 1 ? NPHIP_W1_OCC2_MAX : NPHIP_RW_OCC2_MAX); }
template <bool FUSED, int W, int NV, bool LEAN, bool REMOTE, bool LR, bool WIDE>
constexpr int min_waves() { return LEAN ? NPHIP_LEAN_OCC(W) : (two_waves_per_simd(W, NV, LR, WIDE) ? 2 : ((!FUSED && NV == 0 && !REMOTE) ? NPHIP_CB_OCC(W) : 1)); }
template <bool FUSED, int W, int NV, bool LEAN, bool REMOTE, bool LR, bool WIDE>
constexpr int max_waves() { return LEAN ? NPHIP_LEAN_OCC(W) : (two_waves_per_simd(W, NV, LR, WIDE) ? 2 : 8); }

// Developer builds: -DNPHIP_ONLY_FAMILY=<a name of Family> [-DNPHIP_ONLY_W=<waves>] [-DNPHIP_ONLY_NV=<chunks>] compiles that family alone
// (one instantiation with both: seconds instead of minutes); every other launcher returns hipErrorInvalidValue.
#ifdef NPHIP_ONLY_FAMILY
#ifndef NPHIP_ONLY_W
#define NPHIP_ONLY_W 0
#endif
#ifndef NPHIP_ONLY_NV
#define NPHIP_ONLY_NV -1000
#endif
constexpr bool built(const KernelFamily& f, int W, int nv) {
    return f.family == Family::NPHIP_ONLY_FAMILY && (NPHIP_ONLY_W == 0 || W == NPHIP_ONLY_W) && (NPHIP_ONLY_NV == -1000 || nv == NPHIP_ONLY_NV);
}
#else
constexpr bool built(const KernelFamily&, int, int) { return true; }
#endif

// f(std::integral_constant<int, v>) for the v of the list that equals the run-time value; false when there is none.  (The compiler
// instantiates f for the list's values last to first, and emits the kernels in that order: the lists run downwards, so that a
// translation unit holds its kernels in ascending order.)
template <int... V, class F>
bool dispatch_value(int v, F&& f) { return ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...); }
template <int HI, int... I, class F>
bool dispatch_down_from(int v, std::integer_sequence<int, I...>, F&& f) { return dispatch_value<(HI - I)...>(v, f); }
template <int LO, int HI, class F>
bool dispatch_range(int v, F&& f) { return dispatch_down_from<HI>(v, std::make_integer_sequence<int, HI - LO + 1>{}, f); }

}  // namespace nphip
