// The split-attention gate's shared device code: fc1' + ReLU of one image, ONE function for the forward (fold.hip
// sa_gate_fwd_kernel) and the backward (fold_bwd.hip sa_gate_bwd_kernel), so that the hidden activation the backward masks
// with is, bit for bit, the one the forward fed fc2.
#pragma once
#include "common.h"

#define GATE_MAX_CP 512
#define GATE_THREADS 256

// sum_k x[k] * w[k * ld] over k0 <= k < k1, k1 - k0 a multiple of 8: eight interleaved fmaf chains combined as a fixed tree
__device__ __forceinline__ float gate_dot(const float* __restrict__ x, const float* __restrict__ w, int ld, int k0, int k1) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = k0; k < k1; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = __builtin_fmaf(x[k + u], w[(long)(k + u) * ld], acc[u]);
    }
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// s_h[j] = relu(s_gap . w1[:, j] + b1[j]), j < A, by the whole workgroup of GATE_THREADS threads: GATE_THREADS / A slices of
// the Cp input channels per output column, added in slice order.  s_gap must be visible (a barrier behind its stores); s_h
// is visible to every thread on return.
__device__ __forceinline__ void gate_hidden(const float* __restrict__ s_gap, const float* __restrict__ w1,
                                            const float* __restrict__ b1, float* __restrict__ s_part,
                                            float* __restrict__ s_h, int Cp, int A, int tid) {
    const int parts = GATE_THREADS / A, j = tid % A, p = tid / A, chunk = Cp / parts;
    s_part[tid] = gate_dot(s_gap, w1 + j, A, p * chunk, (p + 1) * chunk);
    __syncthreads();
    if (tid < A) {
        float h = s_part[tid];
        for (int q = 1; q < parts; ++q) h += s_part[q * A + tid];
        s_h[tid] = fmaxf(h + b1[tid], 0.f);
    }
    __syncthreads();
}

// the shapes both gate kernels cover: every slice of fc1's K and fc2's K = A are walked eight channels at a time
static inline bool gate_shape_ok(int Cp, int A) {
    return (A == 32 || A == 64 || A == 128 || A == 256) && Cp <= GATE_MAX_CP && Cp % (8 * (GATE_THREADS / A)) == 0;
}
