// Inference with frozen BatchNorm statistics (include/scouter_hip.h "BatchNorm-folded inference"):
//   scouter_bn_fold_multi     every (convolution, BatchNorm) pair of a model folded into fp32 HWIO weights + biases, ONE launch
//   scouter_sa_gate_fwd_f32   the split-attention gate fc1' -> ReLU -> fc2 -> radix softmax of one image per workgroup
// Plain C++, vector stores only.
#include "common.h"
#include "sa_gate.h"

// ---------------------------------------------------------------------------------------------------------------
// fold: s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s (+ conv_bias * s); products in fp64, rounded once
// ---------------------------------------------------------------------------------------------------------------
struct BnFoldRow {
    const float* w; const float* conv_bias; const float* gamma; const float* beta; const float* mean; const float* var;
    double eps;
    float* w_out; float* bias_out;
    int rows, cout;          // rows = taps * Cin / groups: the HWIO weight is [rows][cout]
    long first;              // running element count (a multiple of 4: cout is)
};

__device__ __forceinline__ double fold_scale(const BnFoldRow& R, int co) {
    return (double)R.gamma[co] / sqrt((double)R.var[co] + R.eps);
}

__global__ __launch_bounds__(256) void bn_fold_multi_kernel(const BnFoldRow* __restrict__ rows, int nrows, long total) {
    const long n4 = total >> 2;
    for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += (long)gridDim.x * blockDim.x) {
        const long e = i4 << 2;
        int lo = 0, hi = nrows - 1;                       // last row with first <= e
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rows[mid].first <= e) lo = mid; else hi = mid - 1;
        }
        const BnFoldRow R = rows[lo];
        const long j = e - R.first;                       // element of this tensor; four consecutive output channels
        const int co = (int)(j % R.cout);
        const f32x4 w = *(const f32x4*)(R.w + j);
        f32x4 o, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double s = fold_scale(R, co + k);
            o[k] = (float)((double)w[k] * s);
            double bb = (double)R.beta[co + k] - (double)R.mean[co + k] * s;
            if (R.conv_bias) bb += (double)R.conv_bias[co + k] * s;
            b[k] = (float)bb;
        }
        *(f32x4*)(R.w_out + j) = o;
        if (j < R.cout) *(f32x4*)(R.bias_out + co) = b;   // (the tensor's first weight row also writes the bias)
    }
}

extern "C" size_t scouter_bn_fold_row_bytes(void) { return sizeof(BnFoldRow); }

extern "C" int scouter_bn_fold_multi(const void* table, int nrows, long total, void* stream) {
    SC_REQUIRE(table && nrows > 0 && total > 0, "bn_fold_multi: bad arguments");
    SC_UNSUPPORTED((total & 3) == 0, "bn_fold_multi: every tensor needs 4-multiples of output channels (total %ld)", total);
    long nb = ((total >> 2) + 255) / 256;
    if (nb > 4096) nb = 4096;
    ScProfScope prof("bn_fold_multi", (hipStream_t)stream, 2.0 * (double)total, 8.0 * (double)total);
    hipLaunchKernelGGL(bn_fold_multi_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const BnFoldRow*)table,
                       nrows, total);
    return sc_check_launch("bn_fold_multi");
}

// ---------------------------------------------------------------------------------------------------------------
// split-attention gate (timm/models/layers/split_attn.py:68-75 with bn1 folded into fc1)
// ---------------------------------------------------------------------------------------------------------------
// one workgroup per image: the result of an image depends on its own row of `gap` only, in one fixed summation order
__global__ __launch_bounds__(GATE_THREADS) void sa_gate_fwd_kernel(const float* __restrict__ gap, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                                   const float* __restrict__ b2, float* __restrict__ a, int Cp,
                                                                   int A) {
    __shared__ float s_gap[GATE_MAX_CP];
    __shared__ float s_part[GATE_THREADS];
    __shared__ float s_h[GATE_THREADS];
    __shared__ float s_z[2 * GATE_MAX_CP];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int c = tid; c < Cp; c += GATE_THREADS) s_gap[c] = gap[(long)b * Cp + c];
    __syncthreads();
    // fc1' + ReLU (sa_gate.h: the function the backward re-forms the hidden activation with)
    gate_hidden(s_gap, w1, b1, s_part, s_h, Cp, A, tid);
    // fc2
    for (int n = tid; n < 2 * Cp; n += GATE_THREADS) s_z[n] = gate_dot(s_h, w2 + n, 2 * Cp, 0, A) + b2[n];
    __syncthreads();
    // radix softmax over the pair (c, Cp + c): the expression of radix_softmax_fwd_kernel (misc_ops.hip)
    for (int c = tid; c < Cp; c += GATE_THREADS) {
        const float z0 = s_z[c], z1 = s_z[Cp + c];
        const float m = fmaxf(z0, z1), e0 = expf(z0 - m), e1 = expf(z1 - m), inv = 1.f / (e0 + e1);
        a[(long)b * 2 * Cp + c] = e0 * inv;
        a[(long)b * 2 * Cp + Cp + c] = e1 * inv;
    }
}

extern "C" int scouter_sa_gate_fwd_f32(const float* gap, const float* w1, const float* b1, const float* w2, const float* b2,
                                       float* a, int B, int Cp, int A, void* stream) {
    SC_REQUIRE(gap && w1 && b1 && w2 && b2 && a && B > 0 && Cp > 0 && A > 0, "sa_gate_fwd: null pointer or empty shape");
    SC_UNSUPPORTED(gate_shape_ok(Cp, A),
                   "sa_gate_fwd: covers attention widths 32 / 64 / 128 / 256 and up to %d channels in multiples of 8 per slice "
                   "(got Cp %d, width %d)", GATE_MAX_CP, Cp, A);
    ScProfScope prof("sa_gate_fwd", (hipStream_t)stream, 6.0 * B * Cp * A, 4.0 * (3.0 * B * Cp + 3.0 * Cp * A));
    hipLaunchKernelGGL(sa_gate_fwd_kernel, dim3((unsigned)B), dim3(GATE_THREADS), 0, (hipStream_t)stream, gap, w1, b1, w2, b2, a,
                       Cp, A);
    return sc_check_launch("sa_gate_fwd");
}
