// drive_plan.h — how the host drives a job, as one pure function of the model and the request.
//
// choose_drive() decides the mode (which loop of host.hip runs the job), the groups of chains and everything else that is a rule and not
// a resource; nphip_sampler::setup() acquires what the plan needs.  A mode or a grouping rule is added here and nowhere else.  Plain C++,
// no HIP: tests/test_host_logic.py pins it on the CPU (nphip_test_choose_drive).
#pragma once
#include <algorithm>
#include <cstdint>

#include "kernel_families.h"

namespace nphip {

enum class Drive : int {
    in_kernel,        // the evaluation runs inside the engine's kernel: fused models, compiled densities, the dense Gaussian's resident form
    host_sync,        // host callback: one launch per evaluation, the stream synchronised before the rows are evaluated
    host_pipelined,   // host callback: groups of chains on their own streams, one launch per evaluation of a group
    host_resident,    // host callback: ONE launch covers every group and stays for `persist_evals` evaluations (a rendezvous each)
    device,           // device callback on the main stream (steady state replayed from a captured graph when graph_steps > 0)
    device_groups     // device callback: groups of chains on their own streams (parallel branches of the graph when graph_steps > 0)
};
inline constexpr int kMaxGroups = 8;

struct DriveIn {
    int kind = 0;             // 0 fused, 1 host callback, 2 device callback (dense: the dense-precision Gaussian), 3 runtime-compiled density
    bool dense = false;
    uint64_t n = 0, dim = 0;  // local chains, dimension
    int W = 1;                // waves per chain and padded row length, as choose_geometry gave them
    int64_t ld = 0;
    bool manual = false, staging_given = false;   // (staging: the caller handed in all three buffers)
    int host_groups = 0, host_persist = 0, graph_steps = 0;
    bool no_register_kernel = false, low_rank_metric = false, store_divergences = false;   // (the first: after the geometry's verdict)
    int n_pause = 0, cus = 0; // pause draws of the adaptation hook; compute units of the device
};

struct DrivePlan {
    Drive mode = Drive::in_kernel;
    bool zero_copy = false;   // host callbacks: the staging buffers are pinned host memory
    int n_groups = 0;
    uint64_t grp_lo[kMaxGroups + 1] = {};   // group g = chains [grp_lo[g], grp_lo[g + 1])
    int remote_nv = 0;        // host_resident: chunks of 128 dimensions per wave
    int persist_evals = 256;  // host_resident: evaluations of a group per launch
    int64_t fall_back_after = 0;   // tests (host_persist = -N): leave the resident mode after N evaluations
    int graph_steps = 0;      // device callbacks: steps per captured graph (0: no graph)
    unsigned seq_first = 0;   // the first sequence number of a group
};

// `want` groups of chains on whole workgroups (`chains_per_workgroup` chains each; 1: any chain may begin a group): never more groups than
// workgroups, so no group is empty.
inline int group_bounds(uint64_t n, int want, uint64_t chains_per_workgroup, uint64_t* lo) {
    const uint64_t wgs = (n + chains_per_workgroup - 1) / chains_per_workgroup;
    const int groups = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)std::max(want, 1), (uint64_t)kMaxGroups, wgs}));
    for (int g = 0; g < groups; ++g) lo[g] = (wgs * (uint64_t)g / (uint64_t)groups) * chains_per_workgroup;
    lo[groups] = n;
    return groups;
}

inline DrivePlan choose_drive(const DriveIn& in) {
    DrivePlan p;
    const uint64_t n = in.n, dim = in.dim;
    const int W = in.W;
    // what rules out every resident form: the adaptation hook edits control blocks between launches, the divergence record needs the
    // pre-step state in memory, and the low-rank metric has no resident kernel
    const bool launch_per_eval_only = in.no_register_kernel || in.low_rank_metric || in.store_divergences || in.n_pause > 0 || in.host_persist == 1;
    // (the dense Gaussian's evaluation is two kernel launches of the engine's own: always capturable — 16 steps per graph unless told otherwise)
    p.graph_steps = (in.kind == 2 && in.graph_steps > 0) ? in.graph_steps : ((in.dense && in.graph_steps == 0) ? 16 : 0);
    if (in.kind == 0 || in.kind == 3) return p;

    if (in.kind == 1) {
        // Host callbacks with small batches are latency-bound (five copies + a synchronisation per leapfrog): there the staging buffers
        // ARE the pinned host buffers (coherent, GPU-visible on ROCm) and the kernel reads / writes them over PCIe directly.  Larger
        // batches keep device staging + bulk copies.
        // (up to 4 MB of positions per step; 8 MB where resident launches apply — dim <= 1024, <= 1024 chains — which need them)
        const uint64_t zc_limit = (n <= 1024 && dim <= 1024) ? (8u << 20) : (4u << 20);
        p.zero_copy = !in.staging_given && n * dim * 8 <= zc_limit;
        p.mode = Drive::host_sync;
        // pipelining: groups of chains in flight — while the host evaluates the rows of one group the kernel of
        // another runs.  Zero-copy batches only (they are the latency-bound ones); host_groups = 1 turns it off.
        if (!p.zero_copy || in.manual || in.host_groups == 1 || n < 2) return p;
        // measured (profiles/r2_config4_host_callback_pipelining.txt): eight schools, 256 chains: 5.7 -> 6.5 (2 groups) -> 6.7 M
        // leapfrogs/s (4 groups); 1024 chains: 12.3 -> 14.5 -> 16.2.  The rest of a step is fixed latency (launch, the memory-resident
        // kernel's dependent passes, its PCIe reads of the gradients, the flag), which groups overlap with each other but cannot
        // shorten — the resident launches can (profiles/r2_config4_resident_launches.txt: 11.3 and 20 M leapfrogs/s).
        int want = (n >= 128) ? 4 : ((n >= 32) ? 2 : 1);
        if (in.host_groups >= 2 && in.host_groups <= kMaxGroups) want = (int)std::min<uint64_t>((uint64_t)in.host_groups, n);
        // Resident launches: the state in registers (a kernel of the remote families with exactly this row length); every chain of a
        // group must be on the device at once (<= 1024 waves: a quarter of the wave slots).
        // (above 4 MB of positions per step the job is bound by PCIe traffic either way, and launches per evaluation were 15 %
        //  faster at 1024 chains x 1000 dimensions: resident only when asked for)
        p.remote_nv = (int)(in.ld / 128 / W);
        const bool resident = (has(kRemoteW1, W, p.remote_nv) || has(kRemoteWn, W, p.remote_nv)) && (int64_t)p.remote_nv * W * 128 == in.ld &&
                              n * (uint64_t)W <= 1024 && !launch_per_eval_only && (n * dim * 8 <= (4u << 20) || in.host_persist > 1);
        p.persist_evals = in.host_persist > 1 ? in.host_persist : 256;
        if (in.host_persist < 0) { p.fall_back_after = -(int64_t)in.host_persist; p.persist_evals = 7; }
        // (a step of a resident group is ~20 us of device latency — PCIe round trips and one L2 write-back — and ~3 us of host work
        //  per 64 rows: eight groups keep the driver thread busy while seven of them are in flight)
        if (resident && in.host_groups == 0) want = (int)std::max<uint64_t>(1, std::min<uint64_t>(8, n / 8));
        // resident: the chains of a workgroup rendezvous as one (kernels.hip: remote_sync) — bounds on whole workgroups
        p.n_groups = group_bounds(n, want, resident ? (uint64_t)chains_per_group(W) : 1, p.grp_lo);
        p.seq_first = resident ? 1u : 0u;
        p.mode = resident ? Drive::host_resident : Drive::host_pipelined;
        return p;
    }

    p.mode = Drive::device;
    if (in.dense) {
        // The resident form: every chain on the device at once (one workgroup of four chains per CU), state in registers ... when the
        // job is large enough for it: a cluster is formed from workgroups of ONE die (8 of them, workgroups dealt round-robin), and its
        // members share the column tiles of the GEMM — with fewer than half as many workgroups per die as there are tiles (64 columns
        // each) a member computes three or more tiles per round and a launch per evaluation is faster (measured: D = 1000: 128 chains
        // 0.69 against 1.05 M leapfrogs/s, 256 chains 2.38 against 2.00; D = 256: 16 chains 0.28 against 0.52, 64 chains 1.59 against
        // 1.39).  host_persist > 1 forces the resident form.
        const uint64_t members = std::min<uint64_t>(16, std::max<uint64_t>(1, ((n + 3) / 4) / 8)), n_tiles = (dim + 63) / 64;
        const uint64_t tiles_per_member = (n_tiles + members - 1) / members;
        if (has(kDenseResident, W, in.ld / 128) && (n + 3) / 4 <= (uint64_t)std::max(in.cus, 0) && !launch_per_eval_only && in.host_groups < 2 &&
            (tiles_per_member <= 2 || in.host_persist > 1))
            p.mode = Drive::in_kernel;
    }
    // Device callbacks in groups: the chains in `host_groups` contiguous groups, each with a stream of its own on which its k_advance
    // launch and its callback alternate — while one group's callback runs (a GEMM, a torch function) the other group's engine kernel
    // does.  No flag and no host synchronisation: stream order is the only dependency.  Bounds on whole workgroups.
    if (in.host_groups >= 2 && !in.manual && n >= 8) {
        p.n_groups = group_bounds(n, in.host_groups, (uint64_t)chains_per_group(W), p.grp_lo);
        p.mode = Drive::device_groups;
    }
    return p;
}

}  // namespace nphip
