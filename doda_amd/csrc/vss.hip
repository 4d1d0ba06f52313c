// Virtual scan simulation, DATA_AUG.aug_list's `vss`, on the device (include/doda_vss.h).
//
// reference dataset/augmentor/augmentor_utils.py:108-251 runs per sample in DataLoader workers: a 10 cm occupancy image for the
// camera candidates, per view a range mask and open3d's hidden_point_removal (qhull on the spherically flipped points plus the
// camera), then a uniform jitter.  Here the scenes of a batch are SEGMENTS of one array (segments.hpp) and the host (doda_amd.vss)
// makes every random decision from a few bytes per segment.
//
// The hull step is a per-point decision: p_i is a hull vertex iff the 2-D linear program of doda_vss.h is feasible.  One wavefront
// decides one query: the lanes hold 64 constraints at a time, the first violated one is found by ballot, and the re-solve on its
// line is a wave-wide interval intersection over the earlier constraints (Seidel's incremental algorithm in a fixed scattered
// order; every constraint causes at most one re-solve, so it terminates without an iteration cap).  Queries are rows of the key-sorted point array, so the waves
// of a workgroup read the same window from L2.
//
// Precision: fp64 throughout, -ffp-contract=off.  A constraint is built from the DIFFERENCE d = p_i - p_j (exact or nearly so for
// neighbours), so the 2000 m magnitude of the flipped points at radius 1000 does not enter the right-hand sides.
#include "segments.hpp"
#include "../../include/doda_vss.h"

static_assert(DODA_VSS_CHUNK == SEG_CHUNK, "include/doda_vss.h promises the chunk size of segments.hpp");

namespace {
using VssSegs = Segs<DODA_VSS_MAX_SEGMENTS>;
constexpr double VSS_BIG = 1.0e6;                        // the box that stands for the unbounded program
constexpr unsigned VSS_PRIME = 1000003u;                 // a query visits constraint (m * prime) % total as its m-th

struct VssGrid {                                         // launch argument of the flip kernel
    double radius[DODA_VSS_MAX_SEGMENTS];
    double hinv[DODA_VSS_MAX_SEGMENTS];
    int32_t G[DODA_VSS_MAX_SEGMENTS];
    int32_t key_base[DODA_VSS_MAX_SEGMENTS];
};

struct VssWin {                                          // launch argument of the decision kernel
    int32_t n;
    int32_t begin[DODA_VSS_MAX_SEGMENTS + 1];
    int32_t G[DODA_VSS_MAX_SEGMENTS];
    int32_t key_base[DODA_VSS_MAX_SEGMENTS];
    double hinv[DODA_VSS_MAX_SEGMENTS];
    double half[DODA_VSS_MAX_SEGMENTS];
};

struct VssOut { long long base[DODA_VSS_MAX_SEGMENTS]; };

__device__ __forceinline__ int cell_of(double unit, double hinv, int G) {
    int c = (int)((unit + 1.0) * hinv);
    c = c < 0 ? 0 : c;
    return c > G - 1 ? G - 1 : c;                        // (a NaN direction truncates to an arbitrary int: clamped too)
}

__device__ __forceinline__ void frame_point(const float *__restrict__ xyz, int i, const double *v, double f[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = ((double)xyz[(size_t)i * 3 + k] - v[k]) - v[3 + k];
}

__global__ __launch_bounds__(SEG_BLOCK) void vss_bounds(const float *__restrict__ xyz, const int32_t *__restrict__ labels, VssSegs s,
                                                      int ignore, float *__restrict__ part, int32_t *__restrict__ count) {
    __shared__ float sh[SEG_WAVES][6];
    __shared__ int kept;
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x == 0) kept = 0;
    doda_sync();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int mine = 0;
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        if (labels[i] == ignore) continue;
        ++mine;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = xyz[(size_t)i * 3 + k];
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane_id() == 0 && mine) atomicAdd(&kept, mine);
    block_minmax(lo, hi, sh, part + (size_t)blockIdx.x * 6);     // (its barrier publishes `kept`)
    if (threadIdx.x == 0 && kept) atomicAdd(&count[ch.seg], kept);
}

__global__ __launch_bounds__(SEG_BLOCK) void vss_bounds_final(VssSegs s, const float *__restrict__ part, float *__restrict__ bounds) {
    __shared__ float sh[SEG_WAVES][6];
    segment_minmax(s, (int)blockIdx.x, part, sh, bounds);
}

__global__ __launch_bounds__(SEG_BLOCK) void vss_image(const float *__restrict__ xyz, const int32_t *__restrict__ labels, VssSegs s,
                                                     int ignore, int floor_label, int ceiling_label, const double *__restrict__ frame,
                                                     uint8_t *__restrict__ img, long long img_len) {
    __shared__ double f[8];
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x < 8) f[threadIdx.x] = frame[ch.seg * 8 + threadIdx.x];
    doda_sync();
    const long long H = (long long)f[5], W = (long long)f[6], base = (long long)f[7];
    if (H <= 0 || W <= 0) return;                        // (uniform over the workgroup)
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        const int lab = labels[i];
        if (lab == ignore) continue;
        const long long r = (long long)(((double)xyz[(size_t)i * 3] - f[0]) * 10.0 - f[3]) + 1;
        const long long c = (long long)(((double)xyz[(size_t)i * 3 + 1] - f[1]) * 10.0 - f[4]) + 1;
        if (r < 0 || r >= H || c < 0 || c >= W) continue;
        const long long at = base + r * W + c;
        if (at < 0 || at + H * W >= img_len) continue;
        img[at] = 1;
        if (lab != floor_label && lab != ceiling_label) img[at + H * W] = 1;
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void vss_view(const float *__restrict__ xyz, const int32_t *__restrict__ labels, VssSegs s,
                                                    int ignore, const double *__restrict__ view, uint8_t *__restrict__ mask,
                                                    int32_t *__restrict__ count) {
    __shared__ double v[16];
    __shared__ int kept;
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x < 16) v[threadIdx.x] = view[ch.seg * 16 + threadIdx.x];
    if (threadIdx.x == 0) kept = 0;
    doda_sync();
    const bool off = v[9] < 0.0, perspective = v[9] > 0.5;
    int mine = 0;
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        bool t = !off && labels[i] != ignore;
        if (t) {
            double f[3];
            frame_point(xyz, i, v, f);
            const double dot = f[0] * v[6] + f[1] * v[7];
            double zu = v[11], zl = v[12];
            if (perspective) {
                const double along = dot / v[13];
                zu = (v[13] - along) * v[14] + v[8];
                zl = (v[13] - along) * v[15] + v[8];
            }
            t = dot <= v[10] && f[2] < zu && f[2] > zl;
        }
        mask[i] = t ? 1 : 0;
        mine += t ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane_id() == 0 && mine) atomicAdd(&kept, mine);
    doda_sync();
    if (threadIdx.x == 0 && kept) atomicAdd(&count[ch.seg], kept);
}

__global__ __launch_bounds__(SEG_BLOCK) void vss_flip(const float *__restrict__ xyz, VssSegs s, const double *__restrict__ view,
                                                    const uint8_t *__restrict__ mask, VssGrid g, double *__restrict__ flipped,
                                                    int32_t *__restrict__ key) {
    __shared__ double v[16];
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x < 16) v[threadIdx.x] = view[ch.seg * 16 + threadIdx.x];
    doda_sync();
    const double radius = g.radius[ch.seg], hinv = g.hinv[ch.seg];
    const int G = g.G[ch.seg], key_base = g.key_base[ch.seg];
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) {
        if (!mask[i]) { key[i] = DODA_VSS_KEY_NONE; continue; }
        double f[3], q[3], p[3];
        frame_point(xyz, i, v, f);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = f[k] - v[6 + k];
        double n = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        if (n == 0.0) n = 0.0001;
        const double fac = 2.0 * (radius - n);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = q[k] + fac * q[k] / n;
            flipped[(size_t)i * 3 + k] = p[k];
        }
        int c = key_base;
        if (G > 0) {
            const double pn = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
            c += (cell_of(p[0] / pn, hinv, G) * G + cell_of(p[1] / pn, hinv, G)) * G + cell_of(p[2] / pn, hinv, G);
        }
        key[i] = c;
    }
}

// ------------------------------------------------------------------------------------------------ the vertex decision
constexpr int EXT_WAVES = 4;

struct Query {                                           // wave-uniform
    double p[3], ph[3], e1[3], e2[3];
    int row, point;
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}

// constraint of row j on the query: b . t <= a.  false: no constraint (the query itself, or a copy of it with a higher point
// number); *dup: a copy with a lower point number (the query is dropped)
__device__ __forceinline__ bool constraint_of(const Query &q, const double *__restrict__ pts, const int32_t *__restrict__ index, int j,
                                              double *a, double *bx, double *by, bool *dup) {
    if (j == q.row) return false;
    const double d0 = q.p[0] - pts[(size_t)j * 3], d1 = q.p[1] - pts[(size_t)j * 3 + 1], d2 = q.p[2] - pts[(size_t)j * 3 + 2];
    if (d0 == 0.0 && d1 == 0.0 && d2 == 0.0) {
        if (index[j] < q.point) *dup = true;
        return false;
    }
    *a = (q.ph[0] * d0 + q.ph[1] * d1) + q.ph[2] * d2;
    *bx = -((q.e1[0] * d0 + q.e1[1] * d1) + q.e1[2] * d2);
    *by = -((q.e2[0] * d0 + q.e2[1] * d1) + q.e2[2] * d2);
    return true;
}

// The rows a query is tested against: up to nine ranges of the sorted array, concatenated into `total` constraints and visited in
// the order (m * stride) % total, stride a prime that does not divide total.  Seidel's algorithm needs an order that is not the
// spatial one: in cell order nearly every constraint moves the optimum and every move rescans all earlier constraints; in a
// scattered order the expected number of moves is logarithmic and their rescans sum to about two passes.  Wave-uniform but g0.
struct Window {
    int rb[9];                                           // first row of each range
    unsigned pre[9];                                     // constraints before each range
    unsigned total;
    unsigned step;                                       // (64 * stride) % total: from a lane's constraint to its next one
    unsigned g0;                                         // (lane * stride) % total: this lane's first constraint
};

// lane r < 9 holds range r as (first row, length)
__device__ __forceinline__ void make_window(Window &w, int my_rb, int my_len) {
    const int lane = lane_id();
    const int incl = wave_inclusive_sum(lane < 9 ? my_len : 0);
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        w.rb[r] = __shfl(my_rb, r, 64);
        w.pre[r] = (unsigned)(__shfl(incl, r, 64) - __shfl(my_len, r, 64));
    }
    w.total = (unsigned)__shfl(incl, 8, 64);
    unsigned stride = VSS_PRIME;
    if (w.total % stride == 0) stride = 999983u;
    if (w.total % stride == 0) stride = 1000033u;
    w.step = w.total ? (64u * stride) % w.total : 0u;
    w.g0 = w.total ? ((unsigned)lane * stride) % w.total : 0u;
}

__device__ __forceinline__ int row_at(const Window &w, unsigned g) {
    int row = w.rb[0] + (int)g;
#pragma unroll
    for (int r = 1; r < 9; ++r)
        if (g >= w.pre[r]) row = w.rb[r] + (int)(g - w.pre[r]);       // (an empty range shares its prefix with the next: the later wins)
    return row;
}

// Seidel's incremental 2-D LP, minimising t1 + t2 / 2 over the box |t1|, |t2| <= half: true iff feasible.  All lanes of the wave.
__device__ __forceinline__ bool feasible_in_box(const Query &q, const double *__restrict__ pts, const int32_t *__restrict__ index,
                                                const Window &w, double half) {
    const int lane = lane_id();
    double tx = -half, ty = -half;
    unsigned g = w.g0;
    for (unsigned m0 = 0; m0 < w.total; m0 += 64) {
        double a = 0.0, bx = 0.0, by = 0.0;
        bool dup = false;
        const bool act = m0 + lane < w.total && constraint_of(q, pts, index, row_at(w, g), &a, &bx, &by, &dup);
        if (__ballot(dup)) return false;
        int done = -1;                                   // lanes up to `done` have had their re-solve or hold at the optimum
        for (;;) {
            const unsigned long long viol = __ballot(act && lane > done && bx * tx + by * ty > a);
            if (!viol) break;
            const int f = __ffsll((long long)viol) - 1;
            done = f;
            const double af = __shfl(a, f, 64), bfx = __shfl(bx, f, 64), bfy = __shfl(by, f, 64);
            const double bb = bfx * bfx + bfy * bfy;
            if (!(bb > 0.0)) return false;               // 0 . t <= af < 0
            // the optimum moves onto the line bf . t = af: t = t0 + s * dir
            const double len = sqrt(bb), t0x = af * bfx / bb, t0y = af * bfy / bb, dx = -bfy / len, dy = bfx / len;
            double lo = -INFINITY, hi = INFINITY;
            bool bad = false;
            auto clip = [&](double den, double rhs) {    // den * s <= rhs
                if (den > 0.0) hi = fmin(hi, rhs / den);
                else if (den < 0.0) lo = fmax(lo, rhs / den);
                else if (rhs < 0.0) bad = true;
            };
            if (lane == 0) {
                clip(dx, half - t0x);
                clip(-dx, half + t0x);
                clip(dy, half - t0y);
                clip(-dy, half + t0y);
            }
            const unsigned lim = m0 + (unsigned)f;       // every earlier constraint
            unsigned gh = w.g0;
            for (unsigned h0 = 0; h0 < lim; h0 += 64) {
                double ah, hx, hy;
                bool dup2 = false;
                if (h0 + lane < lim && constraint_of(q, pts, index, row_at(w, gh), &ah, &hx, &hy, &dup2))
                    clip(hx * dx + hy * dy, ah - (hx * t0x + hy * t0y));
                gh += w.step;
                if (gh >= w.total) gh -= w.total;
            }
            lo = wave_max(lo);
            hi = wave_min(hi);
            if (__ballot(bad) || !(lo <= hi)) return false;
            const double s2 = dx + 0.5 * dy > 0.0 ? lo : hi;
            tx = t0x + s2 * dx;
            ty = t0y + s2 * dy;
        }
        g += w.step;
        if (g >= w.total) g -= w.total;
    }
    return true;
}

__global__ __launch_bounds__(EXT_WAVES * DODA_WAVE) void vss_extreme(const double *__restrict__ pts, const int32_t *__restrict__ index,
                                                                    VssWin w, const int32_t *__restrict__ cell_start,
                                                                    const int32_t *__restrict__ queries, long long n_queries,
                                                                    int exhaustive, uint8_t *__restrict__ selected,
                                                                    uint8_t *__restrict__ state) {
    const long long qi = (long long)blockIdx.x * EXT_WAVES + (threadIdx.x >> 6);
    if (qi >= n_queries) return;                         // (whole waves leave: no workgroup barrier below)
    const int lane = lane_id();
    Query q;
    q.row = queries ? queries[qi] : (int)qi;
    if (q.row < 0 || q.row >= w.begin[w.n]) return;
    int seg = 0;
    for (int k = 1; k < w.n; ++k)
        if (q.row >= w.begin[k]) seg = k;
    q.point = index[q.row];
#pragma unroll
    for (int k = 0; k < 3; ++k) q.p[k] = pts[(size_t)q.row * 3 + k];
    const double norm = sqrt((q.p[0] * q.p[0] + q.p[1] * q.p[1]) + q.p[2] * q.p[2]);
    int result = 0;
    if (norm > 0.0 && norm < INFINITY) {                 // (a point flipped onto the camera is the camera, never a vertex of its own)
#pragma unroll
        for (int k = 0; k < 3; ++k) q.ph[k] = q.p[k] / norm;
        // tangent basis: e1 = ph x (the axis ph is least aligned with), normalised; e2 = ph x e1
        const double ax = fabs(q.ph[0]), ay = fabs(q.ph[1]), az = fabs(q.ph[2]);
        const int axis = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
        const double u[3] = {axis == 0 ? 1.0 : 0.0, axis == 1 ? 1.0 : 0.0, axis == 2 ? 1.0 : 0.0};
        double c[3] = {q.ph[1] * u[2] - q.ph[2] * u[1], q.ph[2] * u[0] - q.ph[0] * u[2], q.ph[0] * u[1] - q.ph[1] * u[0]};
        const double cn = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) q.e1[k] = c[k] / cn;
        q.e2[0] = q.ph[1] * q.e1[2] - q.ph[2] * q.e1[1];
        q.e2[1] = q.ph[2] * q.e1[0] - q.ph[0] * q.e1[2];
        q.e2[2] = q.ph[0] * q.e1[1] - q.ph[1] * q.e1[0];
        const int G = w.G[seg];
        const bool windowed = !exhaustive && G > 0 && w.half[seg] > 0.0;
        int my_rb = 0, my_len = 0;
        Window win;
        if (windowed) {
            const double hinv = w.hinv[seg];
            const int c0 = cell_of(q.ph[0], hinv, G), c1 = cell_of(q.ph[1], hinv, G), c2 = cell_of(q.ph[2], hinv, G);
            if (lane < 9) {
                const int x = c0 + lane / 3 - 1, y = c1 + lane % 3 - 1;
                if (x >= 0 && x < G && y >= 0 && y < G) {
                    const int z0 = c2 > 0 ? c2 - 1 : 0, z1 = c2 < G - 1 ? c2 + 1 : G - 1;
                    const int k0 = w.key_base[seg] + (x * G + y) * G;
                    my_rb = cell_start[k0 + z0];
                    my_len = cell_start[k0 + z1 + 1] - my_rb;
                }
            }
            make_window(win, my_rb, my_len);
            if (feasible_in_box(q, pts, index, win, w.half[seg])) result = 1;
            else if (feasible_in_box(q, pts, index, win, VSS_BIG)) result = 2;
        } else {
            if (lane == 0) { my_rb = w.begin[seg]; my_len = w.begin[seg + 1] - my_rb; }
            make_window(win, my_rb, my_len);
            result = feasible_in_box(q, pts, index, win, VSS_BIG) ? 1 : 0;
        }
    }
    if (lane == 0) {
        state[q.row] = (uint8_t)result;
        if (result == 1) selected[q.point] = 1;
    }
}

// ------------------------------------------------------------------------------------------------ count and emit
__global__ __launch_bounds__(SEG_BLOCK) void vss_count(const uint8_t *__restrict__ selected, VssSegs s, int32_t *__restrict__ count,
                                                     int32_t *__restrict__ blk_cnt) {
    __shared__ int kept;
    const Chunk ch = chunk_of_block(s);
    if (threadIdx.x == 0) kept = 0;
    doda_sync();
    int mine = 0;
    for (int i = ch.base + threadIdx.x; i < ch.end; i += SEG_BLOCK) mine += selected[i] ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane_id() == 0 && mine) atomicAdd(&kept, mine);
    doda_sync();
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = kept;
        if (kept) atomicAdd(&count[ch.seg], kept);
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void vss_emit(const float *__restrict__ xyz, const double *__restrict__ noise,
                                                    const int32_t *__restrict__ labels, const uint8_t *__restrict__ mask1,
                                                    const uint8_t *__restrict__ mask2, VssSegs s, VssOut o,
                                                    const uint8_t *__restrict__ selected, const int32_t *__restrict__ blk_cnt,
                                                    float *__restrict__ out_xyz, int32_t *__restrict__ out_labels,
                                                    int32_t *__restrict__ out_index, uint8_t *__restrict__ out_mask1,
                                                    uint8_t *__restrict__ out_mask2, long long out_len) {
    __shared__ Compact cp;
    const Chunk ch = chunk_of_block(s);
    compact_init(cp, ch, true);
    doda_sync();
    const size_t first = blockIdx.x - ch.index;
    int run = compact_before(cp, true, ch.index, [&](int b) { return blk_cnt[first + b]; });
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int i = ch.base + r * SEG_BLOCK + threadIdx.x;
        compact_round(cp, run, i < ch.end && selected[i] != 0, [&](int rank) {
            const long long row = o.base[ch.seg] + rank;
            if (row < 0 || row >= out_len) return;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = xyz[(size_t)i * 3 + k];
                out_xyz[(size_t)row * 3 + k] = noise ? (float)((double)x + noise[(size_t)i * 3 + k]) : x;
            }
            out_labels[row] = labels[i];
            out_index[row] = i;
            if (mask1) { out_mask1[row] = mask1[i]; out_mask2[row] = mask2[i]; }
        });
    }
}
}  // namespace

extern "C" int32_t doda_vss_abi_version(void) { return DODA_VSS_ABI_VERSION; }

extern "C" int64_t doda_vss_blocks(const int64_t *offsets_h, int32_t n_seg) {
    VssSegs s;
    if (make_segs(offsets_h, n_seg, &s) != DODA_OK) return -1;
    return s.blk[n_seg];
}

extern "C" int doda_vss_bounds(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, int32_t ignore_label,
                               float *part, float *bounds, int32_t *count, doda_stream_t stream) {
    VssSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (!bounds || !count) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    if (nb > 0) {
        if (!xyz || !labels || !part) return DODA_ERR_INVALID;
        hipLaunchKernelGGL(vss_bounds, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, labels, s, (int)ignore_label, part, count);
    }
    hipLaunchKernelGGL(vss_bounds_final, dim3(n_seg), dim3(SEG_BLOCK), 0, as_stream(stream), s, (const float *)part, bounds);
    return doda_check_launch();
}

extern "C" int doda_vss_image(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, int32_t ignore_label,
                              int32_t floor_label, int32_t ceiling_label, const double *frame, uint8_t *img, int64_t img_len,
                              doda_stream_t stream) {
    VssSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (img_len < 0) return DODA_ERR_INVALID;
    const int nb = s.blk[n_seg];
    if (nb == 0 || img_len == 0) return DODA_OK;
    if (!xyz || !labels || !frame || !img) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(vss_image, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, labels, s, (int)ignore_label, (int)floor_label,
                       (int)ceiling_label, frame, img, (long long)img_len);
    return doda_check_launch();
}

extern "C" int doda_vss_view(const float *xyz, const int32_t *labels, const int64_t *offsets_h, int32_t n_seg, int32_t ignore_label,
                             const double *view, uint8_t *mask, int32_t *count, doda_stream_t stream) {
    VssSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !labels || !view || !mask || !count) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(vss_view, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, labels, s, (int)ignore_label, view, mask, count);
    return doda_check_launch();
}

extern "C" int doda_vss_flip(const float *xyz, const int64_t *offsets_h, int32_t n_seg, const double *view, const uint8_t *mask,
                             const double *grid_h, double *flipped, int32_t *key, doda_stream_t stream) {
    VssSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (!grid_h) return DODA_ERR_INVALID;
    VssGrid g = {};
    for (int k = 0; k < n_seg; ++k) {
        const double *r = grid_h + 4 * k;
        if (!(r[0] > 0.0) || !(r[2] >= 0.0) || !(r[3] >= 0.0) || !(r[3] < 2147483647.0)) return DODA_ERR_INVALID;
        if (r[2] > DODA_VSS_MAX_GRID) return DODA_ERR_UNSUPPORTED;
        g.radius[k] = r[0];
        g.hinv[k] = r[1];
        g.G[k] = (int32_t)r[2];
        g.key_base[k] = (int32_t)r[3];
        if (r[3] + r[2] * r[2] * r[2] >= 2147483647.0) return DODA_ERR_UNSUPPORTED;
        if (g.G[k] > 0 && !(r[1] > 0.0)) return DODA_ERR_INVALID;
    }
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !view || !mask || !flipped || !key) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(vss_flip, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, s, view, mask, g, flipped, key);
    return doda_check_launch();
}

extern "C" int doda_vss_extreme(const double *pts, const int32_t *index, const int32_t *seg_begin_h, int32_t n_seg,
                                const int32_t *cell_start, const double *win_h, const int32_t *queries, int64_t n_queries,
                                int32_t flags, uint8_t *selected, uint8_t *state, doda_stream_t stream) {
    if (!seg_begin_h || !win_h || n_seg < 1 || n_queries < 0 || (flags & ~DODA_VSS_EXHAUSTIVE)) return DODA_ERR_INVALID;
    if (n_seg > DODA_VSS_MAX_SEGMENTS) return DODA_ERR_UNSUPPORTED;
    if (seg_begin_h[0] != 0) return DODA_ERR_INVALID;
    const bool exhaustive = (flags & DODA_VSS_EXHAUSTIVE) != 0;
    VssWin w = {};
    w.n = n_seg;
    bool any_window = false;
    for (int k = 0; k < n_seg; ++k) {
        if (seg_begin_h[k + 1] < seg_begin_h[k]) return DODA_ERR_INVALID;
        const double *r = win_h + 4 * k;
        if (!(r[0] >= 0.0) || !(r[3] >= 0.0) || !(r[3] < 2147483647.0)) return DODA_ERR_INVALID;
        if (r[0] > DODA_VSS_MAX_GRID) return DODA_ERR_UNSUPPORTED;
        w.begin[k] = seg_begin_h[k];
        w.G[k] = (int32_t)r[0];
        w.hinv[k] = r[1];
        w.half[k] = r[2];
        w.key_base[k] = (int32_t)r[3];
        const int rows = seg_begin_h[k + 1] - seg_begin_h[k];
        if (!exhaustive && w.G[k] > 0 && w.half[k] > 0.0 && rows > 0) any_window = true;
    }
    w.begin[n_seg] = seg_begin_h[n_seg];
    const long long M = w.begin[n_seg];
    if (!queries && n_queries != M) return DODA_ERR_INVALID;
    if (n_queries == 0) return DODA_OK;
    if (!pts || !index || !selected || !state || (any_window && !cell_start)) return DODA_ERR_INVALID;
    const long long blocks = (n_queries + EXT_WAVES - 1) / EXT_WAVES;
    if (blocks > 0x7fffffffLL) return DODA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vss_extreme, dim3((unsigned)blocks), dim3(EXT_WAVES * DODA_WAVE), 0, as_stream(stream), pts, index, w, cell_start,
                       queries, (long long)n_queries, exhaustive ? 1 : 0, selected, state);
    return doda_check_launch();
}

extern "C" int doda_vss_count(const uint8_t *selected, const int64_t *offsets_h, int32_t n_seg, int32_t *count, int32_t *blk_cnt,
                              doda_stream_t stream) {
    VssSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!selected || !count || !blk_cnt) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(vss_count, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), selected, s, count, blk_cnt);
    return doda_check_launch();
}

extern "C" int doda_vss_emit(const float *xyz, const double *noise, const int32_t *labels, const uint8_t *mask1, const uint8_t *mask2,
                             const int64_t *offsets_h, int32_t n_seg, const uint8_t *selected, const int32_t *blk_cnt,
                             const int64_t *out_base_h, float *out_xyz, int32_t *out_labels, int32_t *out_index, uint8_t *out_mask1,
                             uint8_t *out_mask2, int64_t out_len, doda_stream_t stream) {
    VssSegs s;
    const int st = make_segs(offsets_h, n_seg, &s);
    if (st != DODA_OK) return st;
    if (!out_base_h || out_len < 0) return DODA_ERR_INVALID;
    if ((mask1 == nullptr) != (mask2 == nullptr) || (mask1 == nullptr) != (out_mask1 == nullptr) ||
        (mask1 == nullptr) != (out_mask2 == nullptr))
        return DODA_ERR_INVALID;
    VssOut o = {};
    for (int k = 0; k < n_seg; ++k) {
        if (out_base_h[k] < 0) return DODA_ERR_INVALID;
        o.base[k] = out_base_h[k];
    }
    const int nb = s.blk[n_seg];
    if (nb == 0) return DODA_OK;
    if (!xyz || !labels || !selected || !blk_cnt || !out_xyz || !out_labels || !out_index) return DODA_ERR_INVALID;
    hipLaunchKernelGGL(vss_emit, dim3(nb), dim3(SEG_BLOCK), 0, as_stream(stream), xyz, noise, labels, mask1, mask2, s, o, selected,
                       blk_cnt, out_xyz, out_labels, out_index, out_mask1, out_mask2, (long long)out_len);
    return doda_check_launch();
}
