// The squared distance of the neighbour queries, shared by the kernels whose results must agree bit for bit: the brute-force sweeps
// (neighbors.hip) and the grid search of the evaluation path (eval.hip).
#pragma once
#include "common.hpp"

// (a-b)*(a-b) + (c-d)*(c-d) + (e-f)*(e-f) exactly as the reference source writes it: each operation rounded to nearest, no FMA
// contraction (explicit __fsub_rn / __fmul_rn / __fadd_rn on top of the build's -ffp-contract=off), so that exact ties resolve
// identically everywhere.
__device__ __forceinline__ float dist2_rn(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
