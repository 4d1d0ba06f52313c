// Sparse-convolution weight gradient:  dw[o][ci][co] = sum_t a[tbl[o][t]][ci] * b[t][co].
// (spconv v1.2 indice_conv_backward's per-offset `Xg^T . dYg` GEMMs; reference call sites
// model/unet_block.py:26,29,48,70,78.)  fp32 and bf16 feature storage from one template.
//
// The contraction runs over ROWS, so both MFMA operands need the row index as their k dimension
// while memory holds channels contiguously: rows go through LDS.  Per block and per step of 64
// rows:  the dY tile [64][TB*16] is loaded once (coalesced) into a shared LDS tile and each wave
// lifts its B fragments into registers; then every wave walks ITS OWN subset of kernel offsets
// (o = wave, wave+4, ...): coalesced read of tbl[o][rows], one contiguous row-slice gather per
// lane into a wave-private LDS tile, transposed fragment reads, MFMAs into that offset's
// accumulators.  Gathers for the next offset are issued before the MFMAs of the current one.
// Offsets with no present row in the step are skipped wave-uniformly.  Accumulators (<= 7 offsets
// x TA x TB 16x16 tiles) live in registers for the whole row chunk; per-chunk partials are reduced
// by a second kernel in fixed order (wgrad_common.hpp wgrad_fold): deterministic, no float atomics.
//
// This file also holds the entry point of every weight gradient, doda_spconv_wgrad_multi: ONE call plan (make_call_plan: the
// class of every job and each class's geometry from the pure host functions of wgrad_plan.hpp, then the workspace and descriptor
// layout) serves the size query and the call, and the four kernel classes — this file's gather-table class (namespace doda_dense) and the three of wgrad_backends.hpp — are
// planned, described and launched through the same three steps.
#include "wgrad_common.hpp"
#include <string.h>
#include <mutex>
#include <vector>

namespace {

constexpr int RT = 64;    // rows per step
constexpr int MAX_OGW = 7;  // offsets per wave (4 waves x 7 >= 27)
constexpr int PAD = 8;    // LDS row padding in elements (bank spread, keeps rows 16-byte aligned)

struct F32 {
    typedef float elem;
    typedef f32x4 frag;
    typedef f32x4 vec;                      // 16-byte global / LDS access unit
    static constexpr int VEC = 4;
    static constexpr int KSTEPS = RT / 4;   // v_mfma_f32_16x16x4_f32: 4 rows per MFMA
    typedef float kfrag;                    // one MFMA operand
    // fragments of all KSTEPS k-steps for the 16 channels starting at col0 (lane = (i, g))
    template <int STRIDE>
    static __device__ __forceinline__ void frags(const elem *tile, int g, int i, int col0, kfrag (&out)[KSTEPS]) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) out[ks] = tile[(ks * 4 + g) * STRIDE + col0 + i];
    }
    static __device__ __forceinline__ f32x4 mma(kfrag a, kfrag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
};

// F32S (round 5): fp32 operands, every 16 rows as TWO v_mfma_f32_16x16x32_bf16 on bf16 head / tail splits made in registers
// (x = hi + lo + e, |e| <= 2^-17 |x|): the k = 32 of an instruction is (4 rows of the lane group) x (head, tail) —
// A = [a_hi | a_lo] against B = [b_hi | b_hi], then against [b_lo | b_lo]: all four partial products, fp32 accumulate.  The
// fp32 matrix rate of this part is 1/16 of bf16 and four v_mfma_f32_16x16x4_f32 per 16 rows were the largest item of the
// fp32 step (4.8 of 13.8 ms of kernels); same LDS reads (one float per lane, row and operand), same bytes.  Used for layers
// of many rows (wgrad_plan.hpp plan_dense); small layers keep the exact chain.
struct F32S : F32 {
    static constexpr int KSTEPS = RT / 16;
    struct kfrag { unsigned hi[2], lo[2]; };
    template <int STRIDE>
    static __device__ __forceinline__ void frags(const elem *tile, int g, int i, int col0, kfrag (&out)[KSTEPS]) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = tile[(ks * 16 + 4 * g + q) * STRIDE + col0 + i];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x2 a = {v[2 * h], v[2 * h + 1]};
                const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2));   // round to nearest even
                const f32x2 res = {a[0] - __uint_as_float(hu << 16), a[1] - __uint_as_float(hu & 0xffff0000u)};   // exact
                out[ks].hi[h] = hu;
                out[ks].lo[h] = __builtin_bit_cast(unsigned, __builtin_convertvector(res, bf16x2));
            }
        }
    }
    static __device__ __forceinline__ f32x4 mma(const kfrag &a, const kfrag &b, f32x4 c) {
        const u32x4 av = {a.hi[0], a.hi[1], a.lo[0], a.lo[1]};
        const u32x4 b1 = {b.hi[0], b.hi[1], b.hi[0], b.hi[1]}, b2 = {b.lo[0], b.lo[1], b.lo[0], b.lo[1]};
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, b1), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, b2), c, 0, 0, 0);
    }
};

struct BF16 {
    typedef unsigned short elem;
    typedef s16x4 frag;
    typedef u32x4 vec;
    static constexpr int VEC = 8;
    static constexpr int KSTEPS = RT / 32;  // v_mfma_f32_16x16x32_bf16: 32 rows per MFMA
    typedef bf16x8 kfrag;
    // Rows are the MFMA k dimension but LDS holds [row][channel]: ds_read_b64_tr_b16 does the 4x16
    // transpose in the LDS crossbar.  Probed on gfx950 (tools/probe/trread.hip): when lane t of a
    // 16-lane group g points at &tile[R + t/4][4*(t&3)] it receives {tile[R+q][t] : q = 0..3}.
    // A 16x16x32 operand wants k = 8g..8g+7 per lane: two reads with R = 8g and R = 8g + 4; the two
    // k-steps are 32 rows apart (immediate offsets).  The asm ends with lgkmcnt(0): hipcc does not
    // count LDS ops issued inside asm.
    template <int STRIDE>
    static __device__ __forceinline__ void frags(const elem *tile, int g, int i, int col0, kfrag (&out)[KSTEPS]) {
        static_assert(KSTEPS == 2, "two k-steps of 32 rows");
        const unsigned addr = (unsigned)(uintptr_t)(tile + (8 * g + (i >> 2)) * STRIDE + col0 + 4 * (i & 3));
        s16x4 lo0, hi0, lo1, hi1;
        asm volatile("ds_read_b64_tr_b16 %0, %4\n\t"
                     "ds_read_b64_tr_b16 %1, %4 offset:%5\n\t"
                     "ds_read_b64_tr_b16 %2, %4 offset:%6\n\t"
                     "ds_read_b64_tr_b16 %3, %4 offset:%7\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(lo0), "=&v"(hi0), "=&v"(lo1), "=&v"(hi1)
                     : "v"(addr), "n"(4 * STRIDE * 2), "n"(32 * STRIDE * 2), "n"(36 * STRIDE * 2)
                     : "memory");
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 k0 = __builtin_shufflevector(lo0, hi0, 0, 1, 2, 3, 4, 5, 6, 7);
        const s16x8 k1 = __builtin_shufflevector(lo1, hi1, 0, 1, 2, 3, 4, 5, 6, 7);
        out[0] = __builtin_bit_cast(bf16x8, k0);
        out[1] = __builtin_bit_cast(bf16x8, k1);
    }
    static __device__ __forceinline__ f32x4 mma(kfrag a, kfrag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// VOK: rows of both operands are 16-byte aligned multiples of 16 bytes.  Then every global access is
// an UNCONDITIONAL 16-byte load from an always-valid address (absent rows read row 0) whose value is
// zeroed by a select: no divergent branch around a load, so hipcc can keep many loads in flight
// (with branches it emitted `s_waitcnt vmcnt(0)` after every single load).
template <class T, int TA, int TB, int OGW, bool VOK>
__device__ __forceinline__ void wgrad_body(const typename T::elem *__restrict__ a, int ca,
                                           const typename T::elem *__restrict__ b, int cb,
                                           const int32_t *__restrict__ tbl, int ld, int K,
                                           int n_rows, int rows_per_chunk, int n_tag,
                                           int n_tbg, int n_og, float *__restrict__ partial, int item) {
    typedef typename T::elem elem;
    typedef typename T::frag frag;
    typedef typename T::kfrag kfrag;
    constexpr int SA = TA * 16 + PAD, SB = TB * 16 + PAD;  // LDS row strides (elements)
    __shared__ __attribute__((aligned(16))) elem b_tile[RT * SB];
    __shared__ __attribute__((aligned(16))) elem a_tile[4][RT * SA];

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    // work item = (row chunk, channel-tile group), group fastest
    const int n_grp = n_tag * n_tbg * n_og;
    const int chunk = item / n_grp;
    int grp = item % n_grp;
    const int tag = grp % n_tag; grp /= n_tag;
    const int tbg = grp % n_tbg;
    const int o_base = (grp / n_tbg) * (4 * OGW);   // this block's group of 4*OGW offsets
    const int ca0 = tag * TA * 16, cb0 = tbg * TB * 16;  // channel slices of this block

    f32x4 acc[OGW][TA][TB];
#pragma unroll
    for (int oo = 0; oo < OGW; ++oo)
#pragma unroll
        for (int x_ = 0; x_ < TA; ++x_)
#pragma unroll
            for (int y_ = 0; y_ < TB; ++y_) acc[oo][x_][y_] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const long long r_begin = (long long)chunk * rows_per_chunk;
    long long r_end = r_begin + rows_per_chunk;
    if (r_end > n_rows) r_end = n_rows;

    elem *my_a = a_tile[wid];

    // one lane's row slice: NVA 16-byte vectors (TA*16 channels)
    typedef typename T::vec vec;
    constexpr int VEC = T::VEC, NVA = TA * 16 / VEC, NVB = TB * 16 / VEC;
    auto load_vec = [&](const elem *p, const elem *safe, int c, int cmax, bool ok) -> vec {
        const bool live = ok && c < cmax;
        if constexpr (VOK) {
            // raw value; the CONSUMER zeroes dead lanes (a select here would make the compiler wait
            // for the load on the spot)
            return *reinterpret_cast<const vec *>(live ? p : safe);
        } else {
            vec v = vec{};
            if (live) {
                elem tmp[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) tmp[q] = (c + q < cmax) ? p[q] : (elem)0;
                v = *reinterpret_cast<const vec *>(tmp);
            }
            return v;
        }
    };
    auto gather_row = [&](int idx, vec (&dst)[NVA]) {
#pragma unroll
        for (int f = 0; f < NVA; ++f) {
            const int c = ca0 + f * VEC;
            dst[f] = load_vec(a + (long long)(idx >= 0 ? idx : 0) * ca + c, a, c, ca, idx >= 0);
        }
    };

    // Software pipeline over the 64-row steps: the dY vectors and the table entries of step n+1 are
    // requested at the start of step n and the gather of its first offset during step n's last one,
    // so a step no longer begins with three dependent memory latencies (dY tile, table, first gather)
    // — measured as the bound of this kernel (20 steps x ~3 us per block at level 1).
    constexpr int NDY = (RT * NVB + 255) / 256;   // dY vectors per thread and step
    vec dy_reg[NDY];
    int idx_n[OGW];
    auto load_dy = [&](long long r0) {
#pragma unroll
        for (int k = 0; k < NDY; ++k) {
            const int e = threadIdx.x + k * 256;
            const int r = e / NVB, f = e - r * NVB;
            const long long row = r0 + r;
            const int c = cb0 + f * VEC;
            dy_reg[k] = load_vec(b + (row < r_end ? row : 0) * cb + c, b, c, cb, e < RT * NVB && row < r_end);
        }
    };
    auto load_idx = [&](long long r0) {
#pragma unroll
        for (int oo = 0; oo < OGW; ++oo) {
            const int o = o_base + wid + 4 * oo;
            const long long row = r0 + lane;
            idx_n[oo] = tbl[(o < K && row < r_end) ? (long long)o * ld + row : 0];   // raw; masked when consumed
        }
    };

    vec rows_cur[NVA], rows_nxt[NVA];
    if (r_begin < r_end) {
        load_dy(r_begin);
        load_idx(r_begin);
        gather_row((o_base + wid < K && r_begin + lane < r_end) ? idx_n[0] : -1, rows_cur);
    }
    for (long long r0 = r_begin; r0 < r_end; r0 += RT) {
        // ---- dY tile (already in registers) -> shared LDS ----
        doda_sync();
#pragma unroll
        for (int k = 0; k < NDY; ++k) {
            const int e = threadIdx.x + k * 256;
            if (e < RT * NVB) {
                const int r = e / NVB, f = e - r * NVB;
                const bool live = r0 + r < r_end && cb0 + f * VEC < cb;
                *reinterpret_cast<vec *>(&b_tile[r * SB + f * VEC]) = (VOK && !live) ? vec{} : dy_reg[k];
            }
        }
        int idx[OGW];
#pragma unroll
        for (int oo = 0; oo < OGW; ++oo)
            idx[oo] = (o_base + wid + 4 * oo < K && r0 + lane < r_end) ? idx_n[oo] : -1;
        const bool more = r0 + RT < r_end;
        if (more) {  // in flight for the whole step
            load_dy(r0 + RT);
            load_idx(r0 + RT);
        }
        doda_sync();
        kfrag bf[TB][T::KSTEPS];
#pragma unroll
        for (int y_ = 0; y_ < TB; ++y_) T::template frags<SB>(b_tile, g, i, y_ * 16, bf[y_]);

        // ---- this wave's offsets ----
#pragma unroll
        for (int oo = 0; oo < OGW; ++oo) {
            // gather for the next offset (or for the first offset of the next step) ahead of the MFMAs
            if (oo + 1 < OGW) gather_row(idx[oo + 1], rows_nxt);
            else if (more) gather_row((o_base + wid < K && r0 + RT + lane < r_end) ? idx_n[0] : -1, rows_nxt);
            if (__ballot(idx[oo] >= 0) != 0ull) {
#pragma unroll
                for (int f = 0; f < NVA; ++f) {
                    const bool live = idx[oo] >= 0 && ca0 + f * VEC < ca;
                    *reinterpret_cast<vec *>(&my_a[lane * SA + f * VEC]) = (VOK && !live) ? vec{} : rows_cur[f];
                }
                // LDS operations of one wave are processed in issue order, so the transposed reads
                // below see the stores above (and the next offset's stores cannot overtake these
                // reads) without a counter wait; only the compiler has to be kept from reordering
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int x_ = 0; x_ < TA; ++x_) {
                    kfrag af[T::KSTEPS];
                    T::template frags<SA>(my_a, g, i, x_ * 16, af);
#pragma unroll
                    for (int ks = 0; ks < T::KSTEPS; ++ks)
#pragma unroll
                        for (int y_ = 0; y_ < TB; ++y_)
                            acc[oo][x_][y_] = T::mma(af[ks], bf[y_][ks], acc[oo][x_][y_]);
                }
                __builtin_amdgcn_wave_barrier();
            }
#pragma unroll
            for (int f = 0; f < NVA; ++f) rows_cur[f] = rows_nxt[f];
        }
    }

    // D[i = ci][j = co]: lane (co = lane&15, g) holds ci = 4g + r
    float *out = partial + (long long)chunk * K * ca * cb;
#pragma unroll
    for (int oo = 0; oo < OGW; ++oo) {
        const int o = o_base + wid + 4 * oo;
        if (o < K) {
#pragma unroll
            for (int x_ = 0; x_ < TA; ++x_)
#pragma unroll
                for (int y_ = 0; y_ < TB; ++y_)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ci = ca0 + x_ * 16 + 4 * g + r, co = cb0 + y_ * 16 + i;
                        if (ci < ca && co < cb)
                            out[((long long)o * ca + ci) * cb + co] = acc[oo][x_][y_][r];
                    }
        }
    }
}

// ---- many layers in one launch --------------------------------------------------------------
// The weight gradients of a network are independent of the rest of the backward pass.  Queued and
// launched together (one launch per kernel variant, one reduce launch), the 71 x 2 launches of a U-Net
// step become ~8, and the coarse levels' small grids run side by side instead of one after another.
struct WJob {            // device descriptor of one layer inside a variant group
    const void *a, *b;
    const int32_t *tbl;
    float *out;          // partials of the job (or dw itself when it has a single row chunk)
    int ca, cb, ld, K, n_rows, rows_per_chunk, n_tag, n_tbg, n_og, blk_end;   // blk_end: inclusive prefix
};
using doda_wgrad::RJob;

template <class T, int TA, int TB, int OGW, bool VOK>
__global__ __launch_bounds__(256) void wgrad_multi_kernel(const WJob *__restrict__ jobs, int n_jobs) {
    const int j = find_job<WJob, &WJob::blk_end>(jobs, n_jobs, (int)blockIdx.x);
    const WJob d = jobs[j];
    const int first = j == 0 ? 0 : jobs[j - 1].blk_end;
    wgrad_body<T, TA, TB, OGW, VOK>((const typename T::elem *)d.a, d.ca, (const typename T::elem *)d.b, d.cb,
                                    d.tbl, d.ld, d.K, d.n_rows, d.rows_per_chunk, d.n_tag, d.n_tbg, d.n_og,
                                    d.out, (int)blockIdx.x - first);
}

// the call's reductions over chunk-major partials (gather-table and pair-list jobs): the shared fold, flat source
__global__ __launch_bounds__(256) void wgrad_reduce_multi(const RJob *__restrict__ jobs, int n_jobs) {
    const int j = find_job<RJob, &RJob::blk_end>(jobs, n_jobs, (int)blockIdx.x);
    const RJob d = jobs[j];
    wgrad_fold((int)blockIdx.x - (j == 0 ? 0 : jobs[j - 1].blk_end), d.R, d.n_quad, d.n_quad, d.dw, d.accumulate,
               [&](long long q) { return d.partial + q; });
}

// The scalar form for element counts that are no multiple of four: 16 element lanes x 16 chunk lanes per block;
// lane r sums chunks r, r+16, ... and the 16 lane sums are added in ascending r (deterministic).
__global__ __launch_bounds__(256) void wgrad_reduce(const float *__restrict__ partial, int R,
                                                    long long n_elem, float *__restrict__ dw,
                                                    int accumulate = 0) {
    __shared__ float part[16][17];
    const int el = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const long long e = (long long)blockIdx.x * 16 + el;
    float s = 0.f;
    if (e < n_elem)
        for (int r = rl; r < R; r += 16) s += partial[(long long)r * n_elem + e];
    part[rl][el] = s;
    doda_sync();
    if (rl == 0 && e < n_elem) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += part[r][el];
        dw[e] = accumulate ? dw[e] + t : t;
    }
}


// ---- host side of the many-layer launch -------------------------------------------------------
static_assert(WP_RT == RT && WP_MAX_OGW == MAX_OGW, "wgrad_plan.hpp restates these constants");

// the plan's instantiation: a walk over the compiled set (wgrad_plan.hpp DenseTiles, dense_compiled), which holds every plan that
// doda_dense::plan lets through
template <class T, WgradPolicy P, class... Tile>
void launch_multi_variant(WgradTiles<Tile...>, const DensePlan &p, int total_blocks, const WJob *jobs_dev, int n, hipStream_t s) {
    const auto go = [&](auto tile) {
        typedef decltype(tile) Tl;
        if constexpr (dense_compiled(P, Tl::TA, Tl::TB, Tl::OGW))
            if (p.TA == Tl::TA && p.TB == Tl::TB && p.OGW == Tl::OGW)
                with_bool(p.vok, [&](auto vok) {
                    hipLaunchKernelGGL((wgrad_multi_kernel<T, Tl::TA, Tl::TB, Tl::OGW, decltype(vok)::value>), dim3(total_blocks), dim3(256), 0, s, jobs_dev, n);
                });
    };
    (go(Tile{}), ...);
}

// pinned staging for the descriptor upload (one per process, grow-only, reuse guarded by an event)
struct Staging {
    std::mutex mu;
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    int ev_dev = -1;   // device the event was created on
    bool pending = false;
};
Staging g_staging;

// The gather-table class behind the classes' interface (wgrad_backends.hpp): it takes every job no other class takes.
namespace doda_dense {

struct Plan {
    std::vector<int> idx;
    std::vector<DensePlan> jp;         // per job of idx
    std::vector<size_t> ws_off;        // its partials inside the class's workspace
    std::vector<char> red;             // 0: its one row chunk overwrites dw itself; 1: the shared fold; 2: the per-layer scalar reduce
    struct Group { int first, count, blocks, rep; };   // one launch per kernel variant; rep: a job of the variant
    std::vector<Group> groups;
    std::vector<int> order, blk_end;   // per descriptor: position in idx, inclusive block prefix inside its group
    int status = DODA_OK;              // DODA_ERR_INVALID: a job this kernel cannot run; DODA_ERR_UNSUPPORTED: a plan outside the compiled set
    size_t partial_bytes = 0, desc_bytes = 0;
    int n_reduce = 0;
};

Plan plan(const doda_wgrad_job *jobs, const std::vector<int> &idx) {
    Plan p;
    p.idx = idx;
    p.jp.resize(idx.size());
    p.ws_off.resize(idx.size());
    p.red.resize(idx.size());
    std::vector<int> keys;
    for (size_t k = 0; k < idx.size(); ++k) {
        DensePlan &jp = p.jp[k];
        const doda_wgrad_job &j = jobs[idx[k]];
        jp.key = -1;
        if (!dense_valid(j)) { p.status = DODA_ERR_INVALID; continue; }
        jp = plan_dense(j, doda_wgrad::switches());
        if (!dense_compiled(jp.policy, jp.TA, jp.TB, jp.OGW) && p.status == DODA_OK) p.status = DODA_ERR_UNSUPPORTED;
        const bool quads = (long long)j.K * j.ca * j.cb % 4 == 0 && (uintptr_t)j.dw % 16 == 0;   // whole float quads
        p.red[k] = !dense_needs_partial(jp, j) ? 0 : quads ? 1 : 2;
        p.ws_off[k] = p.partial_bytes;
        p.partial_bytes += dense_partial_bytes(jp, j);
        p.n_reduce += p.red[k] == 1;
        bool seen = false;
        for (int key : keys) seen |= key == jp.key;
        if (!seen) keys.push_back(jp.key);
    }
    for (int key : keys) {      // descriptors grouped by kernel variant
        Plan::Group g{(int)p.order.size(), 0, 0, -1};
        for (size_t k = 0; k < idx.size(); ++k) {
            if (p.jp[k].key != key) continue;
            if (g.rep < 0) g.rep = (int)k;
            g.blocks += p.jp[k].blocks;
            p.order.push_back((int)k);
            p.blk_end.push_back(g.blocks);
            ++g.count;
        }
        p.groups.push_back(g);
    }
    p.desc_bytes = p.order.size() * sizeof(WJob);
    return p;
}

void write_desc(const Plan &p, const doda_wgrad_job *jobs, char *part, void *desc, std::vector<RJob> &reduce, int *reduce_blocks) {
    WJob *wj = (WJob *)desc;
    for (size_t q = 0; q < p.order.size(); ++q) {
        const int k = p.order[q];
        const DensePlan &jp = p.jp[k];
        const doda_wgrad_job &j = jobs[p.idx[k]];
        WJob d;
        d.a = j.a; d.b = j.b; d.tbl = j.tbl;
        d.out = p.red[k] ? (float *)(part + p.ws_off[k]) : j.dw;
        d.ca = j.ca; d.cb = j.cb; d.ld = j.ld; d.K = j.K; d.n_rows = j.n_rows;
        d.rows_per_chunk = jp.rows_per_chunk; d.n_tag = jp.n_tag; d.n_tbg = jp.n_tbg; d.n_og = jp.n_og;
        d.blk_end = p.blk_end[q];
        wj[q] = d;
    }
    for (size_t k = 0; k < p.idx.size(); ++k)
        if (p.red[k] == 1) doda_wgrad::push_reduce(reduce, reduce_blocks, part + p.ws_off[k], jobs[p.idx[k]], p.jp[k].R);
}

int launch(const Plan &p, const void *desc_dev, hipStream_t s) {
    const WJob *wj_dev = (const WJob *)desc_dev;
    for (const Plan::Group &g : p.groups) {
        const DensePlan &q = p.jp[g.rep];
        char name[64];
        dense_name(q, name, sizeof name);
        doda_wgrad::trace(name, g.blocks, 256, g.count);
        if (q.policy == WP_F32S) launch_multi_variant<F32S, WP_F32S>(DenseTiles{}, q, g.blocks, wj_dev + g.first, g.count, s);
        else if (q.policy == WP_F32) launch_multi_variant<F32, WP_F32>(DenseTiles{}, q, g.blocks, wj_dev + g.first, g.count, s);
        else launch_multi_variant<BF16, WP_BF16>(DenseTiles{}, q, g.blocks, wj_dev + g.first, g.count, s);
    }
    return doda_check_launch();
}

// odd element counts: the per-layer scalar reduce
int launch_scalar_reduce(const Plan &p, const doda_wgrad_job *jobs, char *part, hipStream_t s) {
    for (size_t k = 0; k < p.idx.size(); ++k) {
        const doda_wgrad_job &j = jobs[p.idx[k]];
        const long long n_elem = (long long)j.K * j.ca * j.cb;
        if (p.red[k] != 2) continue;
        doda_wgrad::trace("wgrad_reduce", div_up(n_elem, 16), 256, 1);
        hipLaunchKernelGGL(wgrad_reduce, dim3(div_up(n_elem, 16)), dim3(256), 0, s, (const float *)(part + p.ws_off[k]), p.jp[k].R,
                           n_elem, j.dw, (j.flags & DODA_WGRAD_ACCUMULATE) ? 1 : 0);
    }
    return doda_check_launch();
}

}  // namespace doda_dense

// Everything a call does, decided from the host-side job list alone (identical inputs give an identical plan): the class of
// every job, each class's plan, and where its partials and descriptors lie.
//   workspace:   [dense partials][pairs][tile][wide], every part a multiple of 256 bytes
//   descriptors: [dense WJobs][the shared RJob list: dense, then pairs] 16| [pairs PJobs] 16| [wide WwJobs]
struct CallPlan {
    std::vector<int> cls;
    doda_dense::Plan dense;
    doda_pairs::Plan pairs;
    doda_wdma::Plan tile;
    doda_wwide::Plan wide;
    size_t pairs_part, tile_part, wide_part, part_bytes;   // workspace offsets of the classes' partials; their end
    size_t rj_off, pj_off, ww_off, desc_bytes;             // descriptor offsets (dense: 0); their end
    int n_reduce;
};

CallPlan make_call_plan(const doda_wgrad_job *jobs, int n_jobs) {
    CallPlan cp;
    std::vector<int> of[J_WIDE + 1];
    for (int k = 0; k < n_jobs; ++k) {
        cp.cls.push_back(classify(jobs[k], doda_wgrad::switches()));
        of[cp.cls[k]].push_back(k);
    }
    cp.dense = doda_dense::plan(jobs, of[J_DENSE]);
    cp.pairs = doda_pairs::plan(jobs, of[J_PAIRS]);
    cp.tile = doda_wdma::plan(jobs, of[J_TILE]);
    cp.wide = doda_wwide::plan(jobs, of[J_WIDE]);
    cp.pairs_part = cp.dense.partial_bytes;
    cp.tile_part = cp.pairs_part + cp.pairs.partial_bytes;
    cp.wide_part = cp.tile_part + cp.tile.partial_bytes;
    cp.part_bytes = cp.wide_part + cp.wide.partial_bytes;
    cp.n_reduce = cp.dense.n_reduce + cp.pairs.n_reduce;
    cp.rj_off = cp.dense.desc_bytes;
    cp.pj_off = align_up(cp.rj_off + cp.n_reduce * sizeof(RJob), 16);
    cp.ww_off = align_up(cp.pj_off + cp.pairs.desc_bytes, 16);
    cp.desc_bytes = cp.ww_off + cp.wide.desc_bytes;
    return cp;
}
}  // namespace

WgradSwitches &doda_wgrad::switches() {
    static WgradSwitches sw = wgrad_switches_from_env();
    return sw;
}

extern "C" size_t doda_spconv_wgrad_multi_workspace_bytes(const doda_wgrad_job *jobs_h, int32_t n_jobs) {
    if (!jobs_h || n_jobs <= 0) return 0;
    const size_t total = make_call_plan(jobs_h, n_jobs).part_bytes;
    return total < 256 ? 256 : total;
}

// a bound that covers the descriptors of every plan of n_jobs jobs (a job has descriptors in one class only)
extern "C" size_t doda_spconv_wgrad_multi_desc_bytes(int32_t n_jobs) {
    size_t per = sizeof(WJob) + sizeof(RJob);
    if (per < doda_pairs::desc_bytes_per_job()) per = doda_pairs::desc_bytes_per_job();
    if (per < doda_wwide::desc_bytes_per_job()) per = doda_wwide::desc_bytes_per_job();
    return n_jobs <= 0 ? 0 : align_up((size_t)n_jobs * per + 256, 256);
}

extern "C" int doda_spconv_wgrad_multi(const doda_wgrad_job *jobs_h, int32_t n_jobs, void *ws, size_t ws_bytes,
                                       void *desc_dev, size_t desc_bytes, doda_stream_t stream) {
    if (!jobs_h || n_jobs <= 0 || !ws || !desc_dev) return DODA_ERR_INVALID;
    if (desc_bytes < doda_spconv_wgrad_multi_desc_bytes(n_jobs)) return DODA_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    // Every check comes before the first enqueue: a call that returns an error has left the stream and the caller's
    // gradients untouched.
    CallPlan cp = make_call_plan(jobs_h, n_jobs);
    if (cp.dense.status != DODA_OK) return cp.dense.status;
    if (ws_bytes < cp.part_bytes || desc_bytes < cp.desc_bytes) return DODA_ERR_WORKSPACE;
    char *part = (char *)ws;
    int r_blocks = 0;
    doda_wdma::write_desc(cp.tile, jobs_h, part + cp.tile_part);
    if (cp.desc_bytes > 0) {
        std::lock_guard<std::mutex> lock(g_staging.mu);
        Staging &st = g_staging;
        if (st.pending) { hipEventSynchronize(st.ev); st.pending = false; }
        if (st.cap < cp.desc_bytes) {
            if (st.host) hipHostFree(st.host);
            st.cap = align_up(cp.desc_bytes, 4096) * 2;
            if (hipHostMalloc(&st.host, st.cap, hipHostMallocDefault) != hipSuccess) { st.host = nullptr; st.cap = 0; return DODA_ERR_NOMEM; }
        }
        int cur_dev = 0;
        hipGetDevice(&cur_dev);
        if (st.ev && st.ev_dev != cur_dev) { hipEventDestroy(st.ev); st.ev = nullptr; }   // library used from another device
        if (!st.ev && hipEventCreateWithFlags(&st.ev, hipEventDisableTiming) != hipSuccess) return DODA_ERR_LAUNCH;
        st.ev_dev = cur_dev;
        char *host = (char *)st.host;
        std::vector<RJob> rj;
        doda_dense::write_desc(cp.dense, jobs_h, part, host, rj, &r_blocks);
        doda_pairs::write_desc(cp.pairs, jobs_h, part + cp.pairs_part, host + cp.pj_off, rj, &r_blocks);
        doda_wwide::write_desc(cp.wide, part + cp.wide_part, host + cp.ww_off);
        if (!rj.empty()) memcpy(host + cp.rj_off, rj.data(), rj.size() * sizeof(RJob));
        if (hipMemcpyAsync(desc_dev, st.host, cp.desc_bytes, hipMemcpyHostToDevice, s) != hipSuccess) return DODA_ERR_LAUNCH;
        hipEventRecord(st.ev, s);
        st.pending = true;
    }
    // Order on the stream: the descriptor upload; the memsets of empty jobs; per tile rulebook wgrad_dma16 and its
    // wgrad_dma_reduce; the gather-table kernels; the pair-list kernels; wgrad_wide and wgrad_wide_reduce; one
    // wgrad_reduce_multi for the gather-table and pair-list partials; the scalar reduces.  Every class's kernels come before
    // the reduce that reads their partials.
    const char *desc = (const char *)desc_dev;
    for (int k = 0; k < n_jobs; ++k)
        if (cp.cls[k] == J_ZERO && hipMemsetAsync(jobs_h[k].dw, 0, (size_t)jobs_h[k].K * jobs_h[k].ca * jobs_h[k].cb * 4, s) != hipSuccess)
            return DODA_ERR_LAUNCH;
    int st = doda_wdma::launch(cp.tile, jobs_h, s);
    if (st == DODA_OK) st = doda_dense::launch(cp.dense, desc, s);
    if (st == DODA_OK && !cp.pairs.idx.empty()) st = doda_pairs::launch(cp.pairs, desc + cp.pj_off, s);
    if (st == DODA_OK && cp.wide.n > 0) st = doda_wwide::launch(cp.wide, desc + cp.ww_off, s);
    if (st != DODA_OK) return st;
    if (cp.n_reduce > 0) {
        doda_wgrad::trace("wgrad_reduce_multi", r_blocks, 256, cp.n_reduce);
        hipLaunchKernelGGL(wgrad_reduce_multi, dim3(r_blocks), dim3(256), 0, s, (const RJob *)(desc + cp.rj_off), cp.n_reduce);
        st = doda_check_launch();
        if (st != DODA_OK) return st;
    }
    return doda_dense::launch_scalar_reduce(cp.dense, jobs_h, part, s);
}
