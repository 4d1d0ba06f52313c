// Moves between a sparse tensor's rows and its dense volume (include/doda_spconv.h): SparseConvTensor.dense() and its gradient,
// and from_dense().  Pure data movement: bits are copied, never computed on; nothing here uses an atomic.
//
// Channels-last volume [batch][X][Y][Z][c]: a row is contiguous on both sides, so lanes run over the 16-byte pieces of the rows
// (over single elements where a row is not a whole number of aligned pieces).
//
// Channels-first volume [batch][c][X][Y][Z]: a voxel's channels lie X*Y*Z elements apart.  One lane owns one row: it reads the row
// in 16-byte pieces and writes channel after channel, so a wavefront writes ONE channel of 64 consecutive rows per store — in this
// project's voxel orders consecutive rows are mostly z-neighbours, i.e. neighbouring elements of that channel's plane.  Mapping one
// row's channels across the lanes would make every lane of a store hit a different plane.
//
// from_dense: flag (a cell is active iff any channel is non-zero), per-chunk counts, then the stable compaction of segments.hpp over
// the stored counts — the whole volume is one segment — which numbers the active cells in ascending cell order without a scan
// launch or an atomic cursor, and copies their rows.
#include "common.hpp"
#include "segments.hpp"
#include "../../include/doda_spconv.h"

namespace {

struct DenseGrid {
    int B, X, Y, Z;
};

__device__ __forceinline__ bool dense_in_grid(const int4 q, const DenseGrid g) {
    return (unsigned)q.x < (unsigned)g.B && (unsigned)q.y < (unsigned)g.X && (unsigned)q.z < (unsigned)g.Y && (unsigned)q.w < (unsigned)g.Z;
}

template <typename E, int V>
struct alignas(sizeof(E) * V) DensePiece { E e[V]; };

// ---- channels last: U = one 16-byte piece (uint4) or one element; upr = units per row ------------------------------------------
template <typename U, bool SCATTER>
__global__ __launch_bounds__(256) void dense_rows_cl(U *__restrict__ rows, const int4 *__restrict__ indices, int m, int upr,
                                                     DenseGrid g, U *__restrict__ vol) {
    const long long total = (long long)m * upr;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(e / upr), u = (int)(e - (long long)r * upr);
        const int4 q = indices[r];
        const bool ok = dense_in_grid(q, g);
        const long long cell = (((long long)q.x * g.X + q.y) * g.Y + q.z) * g.Z + q.w;
        if (SCATTER) {
            if (ok) vol[cell * upr + u] = rows[e];
        } else {
            U v = U();
            if (ok) v = vol[cell * upr + u];
            rows[e] = v;
        }
    }
}

// ---- channels first: one lane per row, V elements per piece (V = 1: the scalar route) ---------------------------------------------
template <typename E, int V, bool SCATTER>
__global__ __launch_bounds__(256) void dense_rows_cf(E *__restrict__ rows, const int4 *__restrict__ indices, int m, int c,
                                                     DenseGrid g, E *__restrict__ vol) {
    typedef DensePiece<E, V> P;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int4 q = indices[r];
    const bool ok = dense_in_grid(q, g);
    if (SCATTER && !ok) return;
    const long long plane = (long long)g.X * g.Y * g.Z;
    const long long sp = ((long long)q.y * g.Y + q.z) * g.Z + q.w;
    E *v = ok ? vol + (long long)q.x * c * plane + sp : vol;
    E *row = rows + (long long)r * c;
    for (int ch = 0; ch < c; ch += V) {
        P piece;
        if (SCATTER) {
            piece = *reinterpret_cast<const P *>(row + ch);
#pragma unroll
            for (int k = 0; k < V; ++k) v[(long long)(ch + k) * plane] = piece.e[k];
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) piece.e[k] = ok ? v[(long long)(ch + k) * plane] : (E)0;
            *reinterpret_cast<P *>(row + ch) = piece;
        }
    }
}

// ---- from_dense -------------------------------------------------------------------------------------------------------------------
// non-zero test on the bits: everything but the sign (-0 is zero, NaN is not)
__device__ __forceinline__ bool dense_nonzero(uint32_t v) { return (v & 0x7fffffffu) != 0; }
__device__ __forceinline__ bool dense_nonzero(uint16_t v) { return (v & 0x7fffu) != 0; }

template <typename E>
__device__ __forceinline__ bool cell_active(const E *__restrict__ vol, long long cell, int c) {
    const E *p = vol + cell * c;
    bool any = false;
    for (int ch = 0; ch < c; ++ch) any |= dense_nonzero(p[ch]);
    return any;
}

typedef Segs<1> OneSeg;

template <typename E>
__global__ __launch_bounds__(SEG_BLOCK) void from_dense_count(const E *__restrict__ vol, int c, OneSeg s, int32_t *__restrict__ counts) {
    __shared__ int wcnt[SEG_WAVES];
    const Chunk ch = chunk_of_block(s);
    int kept = 0;
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int cell = ch.base + r * SEG_BLOCK + threadIdx.x;
        const bool keep = cell < ch.end && cell_active(vol, cell, c);
        kept += __popcll(__ballot(keep));
    }
    if (lane_id() == 0) wcnt[threadIdx.x >> 6] = kept;
    doda_sync();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < SEG_WAVES; ++w) total += wcnt[w];
        counts[blockIdx.x] = total;
    }
}

// one workgroup: *total = sum of the chunk counts (integers: exact in any order)
__global__ __launch_bounds__(SEG_BLOCK) void from_dense_total(const int32_t *__restrict__ counts, int n, int32_t *__restrict__ total) {
    __shared__ int wsum[SEG_WAVES];
    int local = 0;
    for (int p = threadIdx.x; p < n; p += SEG_BLOCK) local += counts[p];
    local = wave_inclusive_sum(local);
    if (lane_id() == 63) wsum[threadIdx.x >> 6] = local;
    doda_sync();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < SEG_WAVES; ++w) t += wsum[w];
        *total = t;
    }
}

template <typename E>
__global__ __launch_bounds__(SEG_BLOCK) void from_dense_emit(const E *__restrict__ vol, int c, OneSeg s, DenseGrid g,
                                                             const int32_t *__restrict__ counts, int m_out,
                                                             int4 *__restrict__ indices, E *__restrict__ rows) {
    __shared__ Compact cp;
    const Chunk ch = chunk_of_block(s);
    compact_init(cp, ch, true);
    doda_sync();
    int run = compact_before(cp, true, ch.index, [&](int p) { return counts[p]; });
    for (int r = 0; r < SEG_ROUNDS; ++r) {
        const int cell = ch.base + r * SEG_BLOCK + threadIdx.x;
        const bool keep = cell < ch.end && cell_active(vol, cell, c);
        compact_round(cp, run, keep, [&](int row) {
            if (row >= m_out) return;                    // (a volume that changed between the two calls: never out of bounds)
            int rest = cell;
            const int z = rest % g.Z; rest /= g.Z;
            const int y = rest % g.Y; rest /= g.Y;
            const int x = rest % g.X; rest /= g.X;
            indices[row] = make_int4(rest, x, y, z);
            const E *src = vol + (long long)cell * c;
            E *dst = rows + (long long)row * c;
            for (int k = 0; k < c; ++k) dst[k] = src[k];
        });
    }
}

// shape_h -> grid and cell count; DODA_OK or the status
int dense_grid(int32_t batch, const int32_t *shape_h, DenseGrid *g, long double *cells) {
    if (!shape_h || batch < 1 || shape_h[0] < 1 || shape_h[1] < 1 || shape_h[2] < 1) return DODA_ERR_INVALID;
    *g = DenseGrid{batch, shape_h[0], shape_h[1], shape_h[2]};
    *cells = (long double)batch * shape_h[0] * shape_h[1] * shape_h[2];
    return DODA_OK;
}

int move_grid(long long total) { return (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384); }

template <bool SCATTER>
int dense_move(void *rows, const int32_t *indices, int32_t m, int32_t c, int32_t elem_bytes, int32_t batch, const int32_t *shape_h,
               int32_t channels_first, void *volume, doda_stream_t stream) {
    if (m < 0 || c <= 0) return DODA_ERR_INVALID;
    DenseGrid g;
    long double cells;
    const int st = dense_grid(batch, shape_h, &g, &cells);
    if (st != DODA_OK) return st;
    if (elem_bytes != 2 && elem_bytes != 4) return DODA_ERR_UNSUPPORTED;
    if (cells * c * elem_bytes >= 4.0e18L || !volume || (m > 0 && (!rows || !indices))) return DODA_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    if (SCATTER) hipMemsetAsync(volume, 0, (size_t)((long long)cells * c * elem_bytes), s);
    if (m == 0) return doda_check_launch();
    const bool vec = ((long long)c * elem_bytes) % 16 == 0 && al16(rows) && (channels_first || al16(volume));
    const int4 *idx = (const int4 *)indices;
    if (!channels_first) {
        if (vec) {
            const int upr = c * elem_bytes / 16;
            hipLaunchKernelGGL((dense_rows_cl<uint4, SCATTER>), dim3(move_grid((long long)m * upr)), dim3(256), 0, s, (uint4 *)rows, idx, m,
                               upr, g, (uint4 *)volume);
        } else if (elem_bytes == 4) {
            hipLaunchKernelGGL((dense_rows_cl<uint32_t, SCATTER>), dim3(move_grid((long long)m * c)), dim3(256), 0, s, (uint32_t *)rows,
                               idx, m, c, g, (uint32_t *)volume);
        } else {
            hipLaunchKernelGGL((dense_rows_cl<uint16_t, SCATTER>), dim3(move_grid((long long)m * c)), dim3(256), 0, s, (uint16_t *)rows,
                               idx, m, c, g, (uint16_t *)volume);
        }
        return doda_check_launch();
    }
    const dim3 grid(div_up(m, 256));
    if (elem_bytes == 4) {
        if (vec) hipLaunchKernelGGL((dense_rows_cf<uint32_t, 4, SCATTER>), grid, dim3(256), 0, s, (uint32_t *)rows, idx, m, c, g, (uint32_t *)volume);
        else hipLaunchKernelGGL((dense_rows_cf<uint32_t, 1, SCATTER>), grid, dim3(256), 0, s, (uint32_t *)rows, idx, m, c, g, (uint32_t *)volume);
    } else {
        if (vec) hipLaunchKernelGGL((dense_rows_cf<uint16_t, 8, SCATTER>), grid, dim3(256), 0, s, (uint16_t *)rows, idx, m, c, g, (uint16_t *)volume);
        else hipLaunchKernelGGL((dense_rows_cf<uint16_t, 1, SCATTER>), grid, dim3(256), 0, s, (uint16_t *)rows, idx, m, c, g, (uint16_t *)volume);
    }
    return doda_check_launch();
}

// the volume as one segment of `cells` cells
int one_segment(long double cells, OneSeg *s) {
    if (cells > (long double)(0x7fffffffLL - SEG_CHUNK)) return DODA_ERR_UNSUPPORTED;   // (cell + SEG_CHUNK stays an int)
    const int64_t off[2] = {0, (int64_t)cells};
    return make_segs<1>(off, 1, s);
}
}  // namespace

extern "C" int32_t doda_spconv_abi_version(void) { return DODA_SPCONV_ABI_VERSION; }

extern "C" int doda_dense_scatter(const void *rows, const int32_t *indices, int32_t m, int32_t c, int32_t elem_bytes, int32_t batch,
                                  const int32_t *shape_h, int32_t channels_first, void *volume, doda_stream_t stream) {
    return dense_move<true>(const_cast<void *>(rows), indices, m, c, elem_bytes, batch, shape_h, channels_first, volume, stream);
}

extern "C" int doda_dense_gather(const void *volume, const int32_t *indices, int32_t m, int32_t c, int32_t elem_bytes, int32_t batch,
                                 const int32_t *shape_h, int32_t channels_first, void *rows, doda_stream_t stream) {
    return dense_move<false>(rows, indices, m, c, elem_bytes, batch, shape_h, channels_first, const_cast<void *>(volume), stream);
}

extern "C" size_t doda_from_dense_workspace_bytes(int64_t cells) {
    if (cells < 1 || cells > 0x7fffffffLL - DODA_SPCONV_DENSE_CHUNK) return 0;
    return align_up((size_t)((cells + DODA_SPCONV_DENSE_CHUNK - 1) / DODA_SPCONV_DENSE_CHUNK) * 4, 256);
}

extern "C" int doda_from_dense_count(const void *volume, int32_t c, int32_t elem_bytes, int32_t batch, const int32_t *shape_h,
                                     int32_t *count_out, void *ws, size_t ws_bytes, doda_stream_t stream) {
    static_assert(SEG_CHUNK == DODA_SPCONV_DENSE_CHUNK, "the header states the chunk of segments.hpp");
    if (c <= 0) return DODA_ERR_INVALID;
    DenseGrid g;
    long double cells;
    int st = dense_grid(batch, shape_h, &g, &cells);
    if (st != DODA_OK) return st;
    if (elem_bytes != 2 && elem_bytes != 4) return DODA_ERR_UNSUPPORTED;
    OneSeg s;
    if ((st = one_segment(cells, &s)) != DODA_OK) return st;
    if (!volume || !count_out || !ws) return DODA_ERR_INVALID;
    if (ws_bytes < doda_from_dense_workspace_bytes((int64_t)cells)) return DODA_ERR_WORKSPACE;
    hipStream_t hs = as_stream(stream);
    const int nb = s.blk[1];
    if (elem_bytes == 4) hipLaunchKernelGGL(from_dense_count<uint32_t>, dim3(nb), dim3(SEG_BLOCK), 0, hs, (const uint32_t *)volume, c, s, (int32_t *)ws);
    else hipLaunchKernelGGL(from_dense_count<uint16_t>, dim3(nb), dim3(SEG_BLOCK), 0, hs, (const uint16_t *)volume, c, s, (int32_t *)ws);
    hipLaunchKernelGGL(from_dense_total, dim3(1), dim3(SEG_BLOCK), 0, hs, (const int32_t *)ws, nb, count_out);
    return doda_check_launch();
}

extern "C" int doda_from_dense_emit(const void *volume, int32_t c, int32_t elem_bytes, int32_t batch, const int32_t *shape_h,
                                    int32_t m_out, int32_t *indices, void *rows, const void *ws, size_t ws_bytes,
                                    doda_stream_t stream) {
    if (c <= 0 || m_out < 0) return DODA_ERR_INVALID;
    DenseGrid g;
    long double cells;
    int st = dense_grid(batch, shape_h, &g, &cells);
    if (st != DODA_OK) return st;
    if (elem_bytes != 2 && elem_bytes != 4) return DODA_ERR_UNSUPPORTED;
    OneSeg s;
    if ((st = one_segment(cells, &s)) != DODA_OK) return st;
    if (!volume || !ws || (m_out > 0 && (!indices || !rows))) return DODA_ERR_INVALID;
    if (ws_bytes < doda_from_dense_workspace_bytes((int64_t)cells)) return DODA_ERR_WORKSPACE;
    if (m_out == 0) return DODA_OK;
    hipStream_t hs = as_stream(stream);
    const int nb = s.blk[1];
    if (elem_bytes == 4) hipLaunchKernelGGL(from_dense_emit<uint32_t>, dim3(nb), dim3(SEG_BLOCK), 0, hs, (const uint32_t *)volume, c, s, g, (const int32_t *)ws, m_out, (int4 *)indices, (uint32_t *)rows);
    else hipLaunchKernelGGL(from_dense_emit<uint16_t>, dim3(nb), dim3(SEG_BLOCK), 0, hs, (const uint16_t *)volume, c, s, g, (const int32_t *)ws, m_out, (int4 *)indices, (uint16_t *)rows);
    return doda_check_launch();
}
