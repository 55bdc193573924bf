// The layer attributions that keep the gradient PER POSITION of the backbone's output (reference captum_vis.py attributes to
// model.layer4 with captum's layer methods): Layer Integrated Gradients, Layer Conductance (Dhamdhere et al. 2018), HiResCAM
// (Draelos & Carin 2020) and LayerCAM (Jiang et al. 2021).  Three kernels, every product and sum in fp64, each with one fixed
// order per output element and no atomics, so two calls give the same bits.  feat / grads NHWC: a position is C consecutive floats.
//
// conductance_accumulate_kernel: acc[e] = fma(g[j][e], f[j + 1][e] - f[j][e], acc[e]) for j = 0 .. r - 2 ascending, one thread per
//   element (or per four consecutive ones), the previous row's features kept in registers: every row is read once.  The fma is
//   explicit, so the bits do not depend on how the loop is unrolled, and a call that starts at the row another call ended at
//   goes on where that one stopped.
// layer_attr_finish_kernel: ONE workgroup of 1024 threads per class.  A wave takes every 16th position; la_position_sum gives it
//   the fp64 sum of the position's C terms, lane 0 rounds it into map[k][p] and adds the unrounded sum to the wave's running
//   total; the 16 totals meet in LDS and are added in wave order into total[k].  The terms go out as attr (fp32) on the way.
// layer_gxa_kernel: one wave per (image, position) through the same la_position_sum, four positions per workgroup.
//
// la_position_sum: lane l adds the terms of the column groups q = l, l + 64, ... (V = 4 channels with 16-byte loads when C is a
//   multiple of 4 and the pointers allow, else 1) in ascending order from 0.0, then the 64 partial sums meet in a butterfly: an
//   order that depends on C and V alone.  Error: below (C / (64 V) + 7) 2^-53 sum|terms|, inside the (C + 2) 2^-53 of any order.
#include "attr_common.h"

constexpr int LA_THREADS = 256;               // conductance_accumulate (a thread per element), layer_gxa (a wave per position)
constexpr int LA_WAVES = LA_THREADS / 64;

static int la_check_features(const char* what, long P, int C) {
    SC_REQUIRE(P > 0 && C > 0, "%s: bad arguments (P %ld positions, C %d channels: each must be at least 1)", what, P, C);
    SC_UNSUPPORTED(P * C < (1L << 31), "%s: features of %ld x %d elements are past the 32-bit offsets", what, P, C);
    return SC_OK;
}

// the fp64 sum over the C channels of one position by ONE WAVE: term(c, t) forms the V terms of channels c .. c + V - 1; valid in
// every lane (all 64 lanes must call it)
template <int V, typename Term>
__device__ __forceinline__ double la_position_sum(Term term, int C) {
    const int lane = threadIdx.x & 63, cols = C / V;          // (V == 4: C is a multiple of 4)
    double a = 0.0;
    for (int q = lane; q < cols; q += 64) {
        double t[V];
        term(q * V, t);
#pragma unroll
        for (int k = 0; k < V; ++k) a += t[k];
    }
    return wave_sum_d(a);
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(LA_THREADS) void conductance_accumulate_kernel(const float* __restrict__ feats,
                                                                            const float* __restrict__ grads,
                                                                            double* __restrict__ acc, int r, long E) {
    const long e = ((long)blockIdx.x * LA_THREADS + threadIdx.x) * V;
    if (e >= E) return;
    double a[V];
    float f0[V];
    at_load<V>(acc + e, a);
    at_load<V, true>(feats + e, f0);
#pragma unroll 4
    for (int j = 0; j + 1 < r; ++j) {                          // (the last row's gradient is not read)
        float g[V], f1[V];
        at_load<V, true>(grads + (long)j * E + e, g);
        at_load<V, true>(feats + (long)(j + 1) * E + e, f1);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            a[k] = fma((double)g[k], (double)f1[k] - (double)f0[k], a[k]);
            f0[k] = f1[k];
        }
    }
    at_store<V>(acc + e, a);
}

extern "C" int scouter_conductance_accumulate_f64(const float* feats, const float* grads, double* acc, int r, int P, int C,
                                                  void* stream) {
    SC_REQUIRE(feats && grads && acc, "conductance_accumulate: null pointer (feats %p, grads %p, acc %p)", (const void*)feats,
               (const void*)grads, (void*)acc);
    SC_REQUIRE((((uintptr_t)feats | (uintptr_t)grads) & 3) == 0 && ((uintptr_t)acc & 7) == 0,
               "conductance_accumulate: misaligned pointer (feats and grads must be 4-byte, acc 8-byte aligned)");
    SC_REQUIRE(r >= 2, "conductance_accumulate: bad arguments (r %d rows: a step needs two)", r);
    if (int rc = la_check_features("conductance_accumulate", P, C)) return rc;
    const long E = (long)P * C;
    SC_UNSUPPORTED((long)r * E < (1L << 31), "conductance_accumulate: a chunk of %d x %ld elements is past the 32-bit offsets", r, E);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && (((uintptr_t)feats | (uintptr_t)grads | (uintptr_t)acc) & 15) == 0;
    ScProfScope prof("conductance_accumulate", st, 3.0 * (r - 1) * (double)E, (8.0 * r - 4.0 + 16.0) * (double)E);
    const dim3 grid((unsigned)sc_cdiv(vec ? E / 4 : E, LA_THREADS));
    if (vec) hipLaunchKernelGGL(conductance_accumulate_kernel<4>, grid, dim3(LA_THREADS), 0, st, feats, grads, acc, r, E);
    else hipLaunchKernelGGL(conductance_accumulate_kernel<1>, grid, dim3(LA_THREADS), 0, st, feats, grads, acc, r, E);
    return sc_check_launch("conductance_accumulate");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(AT_THREADS) void layer_attr_finish_kernel(const float* __restrict__ feat, const float* __restrict__ base,
                                                                       const double* __restrict__ acc, float* __restrict__ map,
                                                                       float* __restrict__ attr, double* __restrict__ total,
                                                                       int P, int C, int path) {
    __shared__ double s_part[AT_WAVES];
    constexpr int V = VEC ? 4 : 1;
    const int k = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long cls = (long)k * P * C;
    double sum = 0.0;                                          // (the wave's positions, ascending; the same in every lane)
    for (int p = wv; p < P; p += AT_WAVES) {
        const long row = (long)p * C;
        const double s = la_position_sum<V>(
            [&](int c, double (&t)[V]) {
                at_load<V>(acc + cls + row + c, t);
                if (path) {
                    float x[V], b[V];
                    at_load<V>(feat + row + c, x);
                    if (base) {
                        at_load<V>(base + row + c, b);
                    } else {
#pragma unroll
                        for (int i = 0; i < V; ++i) b[i] = 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < V; ++i) t[i] = ((double)x[i] - (double)b[i]) * t[i];
                }
                if (attr) {
                    float* __restrict__ o = attr + cls + row + c;
                    if constexpr (VEC) *(f32x4*)o = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
                    else o[0] = (float)t[0];
                }
            },
            C);
        if (lane == 0) map[(long)k * P + p] = (float)s;
        sum += s;
    }
    if (total) {                                               // (uniform over the launch)
        if (lane == 0) s_part[wv] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int i = 0; i < AT_WAVES; ++i) t += s_part[i];
            total[k] = t;
        }
    }
}

extern "C" int scouter_layer_attr_finish_f32(const float* feat, const float* base, const double* acc, float* map, float* attr,
                                             double* total, int K, int P, int C, int mode, void* stream) {
    SC_REQUIRE(mode == 0 || mode == 1, "layer_attr_finish: mode %d (0: path, (feat - base) * acc; 1: sum, acc itself)", mode);
    const bool path = mode == 0;
    SC_REQUIRE(acc && map && (!path || feat), "layer_attr_finish: null pointer (mode %d: feat %p, acc %p, map %p)", mode,
               (const void*)feat, (const void*)acc, (void*)map);
    if (!path) feat = base = nullptr;                          // (ignored in mode sum)
    SC_REQUIRE((((uintptr_t)feat | (uintptr_t)base | (uintptr_t)map | (uintptr_t)attr) & 3) == 0 &&
                   (((uintptr_t)acc | (uintptr_t)total) & 7) == 0,
               "layer_attr_finish: misaligned pointer (feat, base, map and attr must be 4-byte, acc and total 8-byte aligned)");
    SC_REQUIRE(K > 0, "layer_attr_finish: bad arguments (K %d classes must be at least 1)", K);
    if (int rc = la_check_features("layer_attr_finish", P, C)) return rc;
    SC_UNSUPPORTED((long)K * P * C < (1L << 31), "layer_attr_finish: sums of %d x %d x %d elements are past the 32-bit offsets", K, P,
                   C);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && (((uintptr_t)feat | (uintptr_t)base | (uintptr_t)acc | (uintptr_t)attr) & 15) == 0;
    const double E = (double)K * P * C;
    ScProfScope prof("layer_attr_finish", st, 3.0 * E, (8.0 + (path ? (base ? 8.0 : 4.0) : 0.0) + (attr ? 4.0 : 0.0)) * E);
    if (vec)
        hipLaunchKernelGGL(layer_attr_finish_kernel<true>, dim3((unsigned)K), dim3(AT_THREADS), 0, st, feat, base, acc, map, attr,
                           total, P, C, path ? 1 : 0);
    else
        hipLaunchKernelGGL(layer_attr_finish_kernel<false>, dim3((unsigned)K), dim3(AT_THREADS), 0, st, feat, base, acc, map, attr,
                           total, P, C, path ? 1 : 0);
    return sc_check_launch("layer_attr_finish");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(LA_THREADS) void layer_gxa_kernel(const float* __restrict__ feat, const float* __restrict__ dfeat,
                                                               float* __restrict__ out, long BP, int P, int C, long out_stride,
                                                               int rectify, int relu) {
    constexpr int V = VEC ? 4 : 1;
    const long i = (long)blockIdx.x * LA_WAVES + (threadIdx.x >> 6);          // (image, position); uniform over the wave
    if (i >= BP) return;
    const long row = i * C;
    double s = la_position_sum<V>(
        [&](int c, double (&t)[V]) {
            float x[V], g[V];
            at_load<V>(feat + row + c, x);
            at_load<V>(dfeat + row + c, g);
#pragma unroll
            for (int k = 0; k < V; ++k) t[k] = (double)(rectify ? fmaxf(g[k], 0.f) : g[k]) * (double)x[k];
        },
        C);
    if (relu) s = fmax(s, 0.0);
    const long b = i / P;
    if ((threadIdx.x & 63) == 0) out[b * out_stride + (i - b * P)] = (float)s;
}

extern "C" int scouter_layer_gxa_f32(const float* feat, const float* dfeat, float* out, int B, int P, int C, long out_stride,
                                     int rectify, int relu, void* stream) {
    SC_REQUIRE(feat && dfeat && out, "layer_gxa: null pointer (feat %p, dfeat %p, out %p)", (const void*)feat, (const void*)dfeat,
               (void*)out);
    SC_REQUIRE((((uintptr_t)feat | (uintptr_t)dfeat | (uintptr_t)out) & 3) == 0,
               "layer_gxa: misaligned pointer (feat, dfeat and out must be 4-byte aligned)");
    SC_REQUIRE(B > 0, "layer_gxa: bad arguments (B %d images must be at least 1)", B);
    if (int rc = la_check_features("layer_gxa", P, C)) return rc;
    SC_REQUIRE(out_stride >= P || B == 1, "layer_gxa: output batch stride %ld is below P = %d", out_stride, P);
    SC_UNSUPPORTED((long)B * P * C < (1L << 31), "layer_gxa: a batch of %d x %d x %d elements is past the 32-bit offsets", B, P, C);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && (((uintptr_t)feat | (uintptr_t)dfeat) & 15) == 0;
    const long BP = (long)B * P;
    ScProfScope prof("layer_gxa", st, 2.0 * (double)BP * C, 4.0 * (double)BP * (2.0 * C + 1.0));
    const dim3 grid((unsigned)sc_cdiv(BP, LA_WAVES));
    if (vec) hipLaunchKernelGGL(layer_gxa_kernel<true>, grid, dim3(LA_THREADS), 0, st, feat, dfeat, out, BP, P, C, out_stride, rectify,
                                relu);
    else hipLaunchKernelGGL(layer_gxa_kernel<false>, grid, dim3(LA_THREADS), 0, st, feat, dfeat, out, BP, P, C, out_stride, rectify,
                            relu);
    return sc_check_launch("layer_gxa");
}
