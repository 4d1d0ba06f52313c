// Host side of doda_spconv_wgrad_multi: the interface between the call planner (spconv_wgrad.hip) and the four kernel
// classes of the weight gradient.  Not part of the C ABI.
//
// Every class — doda_dense (gather table, spconv_wgrad.hip, file-local), doda_pairs (pair lists, spconv_wgrad_pairs.hip),
// doda_wdma (16 x 16 tiles over a tilebook, spconv_wdma.hip), doda_wwide (wide tiles, spconv_wwide.hip) — shows the planner
// the same three steps:
//   1. plan(jobs, idx): for the call's job indices of the class, in queue order, a Plan that records the launch geometry and
//      how much the class needs: partial_bytes of workspace (a multiple of 256) and, where it has any, desc_bytes of device
//      descriptors and n_reduce entries of the shared reduction list.  Identical inputs give an identical plan.
//   2. write_desc(plan, ..., part, ...): the host copy of the descriptors, given the address of the class's partials.
//   3. launch(plan, ..., s): the class's kernels, given the device address of its descriptors.
// Which class takes a job, and every geometry a plan is made of, is decided in wgrad_plan.hpp (pure host functions of the job
// and the switches: classify, the classes' *_eligible predicates, plan_dense); nothing here or in the classes' files chooses.
#pragma once
#include "common.hpp"
#include "wgrad_plan.hpp"
#include <vector>

namespace doda_wgrad {
// the process-wide switches: the environment once, at the first weight-gradient or option call, then doda_set_option
WgradSwitches &switches();
// DODA_TRACE_WGRAD=1: one line per kernel launch of the call on stderr; `name` as a kernel trace shows it, namespaces stripped
inline void trace(const char *name, unsigned grid, unsigned block, int jobs) {
    if (switches().trace) fprintf(stderr, "wgrad route=%s grid=%u block=%u jobs=%d\n", name, grid, block, jobs);
}
// One fixed-order reduction dw[q] (+)= sum_r partial[r][q] over float quads (wgrad_common.hpp wgrad_fold); every class
// whose partials lie chunk-major appends its reductions to the call's one list, summed by one wgrad_reduce_multi launch.
struct RJob {
    const float4 *partial;
    float4 *dw;
    long long n_quad;
    int R, blk_end, accumulate, pad;   // blk_end: inclusive block prefix inside the launch
};
// chunk lanes of a fold block: the smallest power of two >= min(R, 16); the block then holds 256 / lanes quads
__host__ __device__ inline int reduce_lanes(int R) {
    int rl = 1;
    while (rl < 16 && rl < R) rl *= 2;
    return rl;
}
inline int reduce_blocks(long long n_quad, int R) { return div_up(n_quad, 256 / reduce_lanes(R)); }
// appends a job's reduction; *blocks: the list's running block count
inline void push_reduce(std::vector<RJob> &list, int *blocks, const void *partial, const doda_wgrad_job &j, int R) {
    RJob d;
    d.partial = (const float4 *)partial;
    d.dw = (float4 *)j.dw;
    d.n_quad = (long long)j.K * j.ca * j.cb / 4;
    d.R = R;
    d.accumulate = (j.flags & DODA_WGRAD_ACCUMULATE) ? 1 : 0;
    d.pad = 0;
    d.blk_end = *blocks += reduce_blocks(d.n_quad, R);
    list.push_back(d);
}
}  // namespace doda_wgrad

// Pair-list kernels: bf16, 16-channel multiples, pair lists given or identity, operands inside the 4 GB hardware range check
namespace doda_pairs {
struct Plan {
    std::vector<int> idx;
    std::vector<size_t> part_off;      // per job: its partials inside the class's workspace (unused when it writes dw itself)
    struct Group { int ta, tb, first, count, blocks; };
    std::vector<Group> groups;         // one launch each; `first` = index of the group's first descriptor
    std::vector<int> order, blk_end;   // per descriptor: position in idx, inclusive block prefix inside its group
    size_t partial_bytes = 0, desc_bytes = 0;
    int n_reduce = 0;
};
Plan plan(const doda_wgrad_job *jobs, const std::vector<int> &idx);
void write_desc(const Plan &p, const doda_wgrad_job *jobs, char *part, void *desc, std::vector<doda_wgrad::RJob> &reduce,
                int *reduce_blocks);
int launch(const Plan &p, const void *desc_dev, hipStream_t s);
size_t desc_bytes_per_job();           // descriptor + reduction entry
}  // namespace doda_pairs

// LDS-staged 16 x 16 tile kernel over a tilebook (spconv_wdma.hip): bf16 K = 27 layers of 16 .. 64 channels, one launch per
// rulebook (jobs sharing tilebook, table, row count and leading dimension) and 16 channel blocks.  Its descriptors travel
// in the kernel arguments (no device descriptors): write_desc keeps them in the plan.
namespace doda_wdma {
inline bool enabled() { return doda_wgrad::switches().wdma; }
inline void set_enabled(bool on) { doda_wgrad::switches().wdma = on; }
struct Plan {
    struct Launch { int first_job, n_jobs, n_blocks; size_t part_off; };   // first_job: position in `order`
    std::vector<Launch> launches;
    std::vector<int> order;            // job indices grouped by rulebook
    std::vector<unsigned char> args;   // write_desc: the kernel arguments of every launch
    size_t partial_bytes = 0;
};
Plan plan(const doda_wgrad_job *jobs, const std::vector<int> &idx);
void write_desc(Plan &p, const doda_wgrad_job *jobs, char *part);
int launch(const Plan &p, const doda_wgrad_job *jobs, hipStream_t s);
}  // namespace doda_wdma

// LDS-staged wide tile kernel over a tilebook (spconv_wwide.hip): bf16 K = 27 layers of 48 .. 224 channels, every such job
// of a call in one launch, over the row chunks of the gather-table plan (plan_dense), whose sums the kernel reproduces bit for bit.
namespace doda_wwide {
struct Plan {
    std::vector<unsigned char> desc;   // the descriptors, their partials as offsets into the class's workspace
    int n = 0, wgs = 0, red_blocks = 0;
    size_t partial_bytes = 0, desc_bytes = 0;
};
Plan plan(const doda_wgrad_job *jobs, const std::vector<int> &idx);
void write_desc(const Plan &p, char *part, void *desc);
int launch(const Plan &p, const void *desc_dev, hipStream_t s);
size_t desc_bytes_per_job();
}  // namespace doda_wwide
