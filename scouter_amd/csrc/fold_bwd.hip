// The gradient-only backward of the BatchNorm-folded eval path (include/scouter_hip.h "Backward of the folded path";
// SlotModel.image_pass): the three passes the folded forward has no training counterpart for.
//   scouter_sa_gate_bwd_f32          the split-attention gate's backward, one workgroup per image
//   scouter_sa_apply_relu_bwd_f32    the weighted sum's + GAP's backward with the radix convolution's ReLU mask applied
//   scouter_maxpool_relu_bwd_f32     the max-pool gather with the stem ReLU's mask applied
// and their scouter_*_rule_f32 forms: the rule of relu_rule.h (gradient / guided backpropagation / deconvnet) as a compile-time
// argument of every kernel here; rule 0 is the code of the three entry points above, and rule 2 issues no load of the activation.
// Plain C++, vector stores only, no atomics: every output element has one fixed summation order.
#include "common.h"
#include "relu_rule.h"
#include "sa_gate.h"

// ---------------------------------------------------------------------------------------------------------------
// split-attention gate backward: da -> dgap through radix softmax, fc2, ReLU, fc1'
// ---------------------------------------------------------------------------------------------------------------
// out(r) = sum_n m[r][n] * v[n] for the rows r < nrows of a ROW-MAJOR matrix m [nrows][len] and a vector v [len] in LDS.
// The backward walks fc2's (fc1's) weight against the order the forward read it in: there thread n took column n, here an
// output needs a whole ROW.  The layout chosen keeps the row's own storage order: G = min(64, len / 4 rounded up to a power
// of two) neighbouring lanes read 16-byte pieces of one row (coalesced, no LDS staging of the weight, which is read once), 64 / G
// rows per wave at a time, 4 waves.  Per lane four interleaved fmaf chains over its pieces in ascending order, combined
// (c0 + c1) + (c2 + c3), then a butterfly over the G lanes: the order is a function of (len, G) alone.
template <typename Store>
__device__ __forceinline__ void gate_rows_dot(const float* __restrict__ m, const float* __restrict__ v, int nrows, int len,
                                              int G, int tid, Store store) {
    const int lane = tid & 63, wave = tid >> 6, sub = lane & (G - 1), rpw = 64 / G, rw = lane / G;
    for (int rb = wave * rpw; rb < nrows; rb += (GATE_THREADS / 64) * rpw) {        // (wave-uniform trip count)
        const int r = rb + rw;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (r < nrows) {
            for (int n = 4 * sub; n < len; n += 4 * G) {
                const f32x4 w = *(const f32x4*)(m + (long)r * len + n);
                const f32x4 x = *(const f32x4*)(v + n);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __builtin_fmaf(w[k], x[k], acc[k]);
            }
        }
        float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (sub == 0 && r < nrows) store(r, s);
    }
}

static inline int gate_group(int len) {          // lanes per row: len / 4 pieces, rounded up to a power of two, at most a wave
    int g = 1;
    while (g < 64 && 4 * g < len) g <<= 1;
    return g;
}

template <int RULE>
__global__ __launch_bounds__(GATE_THREADS) void sa_gate_bwd_kernel(const float* __restrict__ gap, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                                   const float* __restrict__ a, const float* __restrict__ da,
                                                                   float* __restrict__ dgap, float* __restrict__ h_out, int Cp,
                                                                   int A, int G2, int G1) {
    __shared__ float s_gap[GATE_MAX_CP];
    __shared__ float s_part[GATE_THREADS];
    __shared__ float s_h[GATE_THREADS];
    __shared__ __attribute__((aligned(16))) float s_dz[2 * GATE_MAX_CP];
    __shared__ __attribute__((aligned(16))) float s_dh[GATE_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int c = tid; c < Cp; c += GATE_THREADS) s_gap[c] = gap[(long)b * Cp + c];
    // radix softmax backward over the pair (c, Cp + c): the expression of radix_softmax_bwd_kernel (misc_ops.hip)
    for (int c = tid; c < Cp; c += GATE_THREADS) {
        const long i0 = (long)b * 2 * Cp + c, i1 = i0 + Cp;
        const float dot = a[i0] * da[i0] + a[i1] * da[i1];
        s_dz[c] = a[i0] * (da[i0] - dot);
        s_dz[Cp + c] = a[i1] * (da[i1] - dot);
    }
    __syncthreads();
    gate_hidden(s_gap, w1, b1, s_part, s_h, Cp, A, tid);             // the forward's hidden activation, bit for bit
    if (h_out && tid < A) h_out[(long)b * A + tid] = s_h[tid];
    // dh[j] = (sum_n dz[n] * w2[j][n]) * [h[j] > 0]   (RULE 0; relu_rule.h for the others)
    gate_rows_dot(w2, s_dz, A, 2 * Cp, G2, tid, [&](int j, float s) { s_dh[j] = relu_rule<RULE>(s, s_h[j]); });
    __syncthreads();
    // dgap[c] = sum_j dh[j] * w1'[c][j]
    gate_rows_dot(w1, s_dh, Cp, A, G1, tid, [&](int c, float s) { dgap[(long)b * Cp + c] = s; });
}

static int sa_gate_bwd_launch(const float* gap, const float* w1, const float* b1, const float* w2, const float* a,
                              const float* da, float* dgap, float* h_out, int B, int Cp, int A, int rule, void* stream) {
    SC_REQUIRE(gap && w1 && b1 && w2 && a && da && dgap && B > 0 && Cp > 0 && A > 0, "sa_gate_bwd: null pointer or empty shape");
    SC_UNSUPPORTED(gate_shape_ok(Cp, A),
                   "sa_gate_bwd: covers attention widths 32 / 64 / 128 / 256 and up to %d channels in multiples of 8 per slice "
                   "(got Cp %d, width %d)", GATE_MAX_CP, Cp, A);
    SC_REQUIRE(((uintptr_t)w1 | (uintptr_t)w2) % 16 == 0, "sa_gate_bwd: the weights are read as 16-byte vectors: unaligned pointer");
    SC_REQUIRE_RULE(rule, "sa_gate_bwd");
    ScProfScope prof("sa_gate_bwd", (hipStream_t)stream, 10.0 * B * Cp * A, 4.0 * (6.0 * B * Cp + 4.0 * Cp * A));
    rule_dispatch(rule, [&](auto r) {
        hipLaunchKernelGGL(sa_gate_bwd_kernel<decltype(r)::value>, dim3((unsigned)B), dim3(GATE_THREADS), 0, (hipStream_t)stream, gap,
                           w1, b1, w2, a, da, dgap, h_out, Cp, A, gate_group(2 * Cp), gate_group(A));
    });
    return sc_check_launch("sa_gate_bwd");
}

extern "C" int scouter_sa_gate_bwd_f32(const float* gap, const float* w1, const float* b1, const float* w2, const float* a,
                                       const float* da, float* dgap, float* h_out, int B, int Cp, int A, void* stream) {
    return sa_gate_bwd_launch(gap, w1, b1, w2, a, da, dgap, h_out, B, Cp, A, RULE_GRADIENT, stream);
}

extern "C" int scouter_sa_gate_bwd_rule_f32(const float* gap, const float* w1, const float* b1, const float* w2, const float* a,
                                            const float* da, float* dgap, float* h_out, int B, int Cp, int A, int rule,
                                            void* stream) {
    return sa_gate_bwd_launch(gap, w1, b1, w2, a, da, dgap, h_out, B, Cp, A, rule, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// dx[b,hw,r*Cp+c] = x0[b,hw,r*Cp+c] > 0 ? dout[b,hw,c] * a[b,r*Cp+c] + dgap[b,c] * (1 / HW) : +0
// (sa_apply_bwd_kernel of misc_ops.hip with the ReLU of the folded radix convolution in the same pass: dout is read once
// for both radix halves, x0 and dx once each, every access 16 bytes: 20 bytes per dout element.  RULE (relu_rule.h) acts on
// g = dout * a_r + dgap / HW, the value formed in front of the mask; rule 2 does not read x0: 12 bytes per dout element)
// ---------------------------------------------------------------------------------------------------------------
template <int RULE>
__global__ __launch_bounds__(256) void sa_apply_relu_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ a,
                                                                const float* __restrict__ dgap, const float* __restrict__ x0,
                                                                float* __restrict__ dx, long n4, int HW, int Cp, float inv_hw) {
    const int c4n = Cp / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        const long row = i / c4n;
        const int b = (int)(row / HW);
        const f32x4 d = __builtin_nontemporal_load((const f32x4*)(dout + i * 4));
        const f32x4 gp = *(const f32x4*)(dgap + (long)b * Cp + c) * inv_hw;
        const f32x4 a0 = *(const f32x4*)(a + (long)b * 2 * Cp + c), a1 = *(const f32x4*)(a + (long)b * 2 * Cp + Cp + c);
        const long o = row * 2 * Cp + c;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if constexpr (rule_reads_activation<RULE>) {
            v0 = __builtin_nontemporal_load((const f32x4*)(x0 + o));
            v1 = __builtin_nontemporal_load((const f32x4*)(x0 + o + Cp));
        }
        f32x4 g0 = d * a0 + gp, g1 = d * a1 + gp;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g0[k] = relu_rule<RULE>(g0[k], v0[k]);
            g1[k] = relu_rule<RULE>(g1[k], v1[k]);
        }
        *(f32x4*)(dx + o) = g0;
        *(f32x4*)(dx + o + Cp) = g1;
    }
}

static inline int fb_blocks(long n) { long b = (n + 255) / 256; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

static int sa_apply_relu_bwd_launch(const float* dout, const float* a, const float* dgap, const float* x0, float* dx, int B,
                                    int HW, int Cp, int rule, void* stream) {
    SC_REQUIRE(dout && a && dgap && x0 && dx && B > 0 && HW > 0 && Cp > 0, "sa_apply_relu_bwd: null pointer or empty shape");
    SC_REQUIRE(Cp % 4 == 0, "sa_apply_relu_bwd: Cp %% 4 != 0");
    SC_REQUIRE_RULE(rule, "sa_apply_relu_bwd");
    const long n4 = (long)B * HW * Cp / 4;
    ScProfScope prof("sa_apply_relu_bwd", (hipStream_t)stream, 0, (rule == RULE_DECONVNET ? 12.0 : 20.0) * (double)B * HW * Cp);
    rule_dispatch(rule, [&](auto r) {
        hipLaunchKernelGGL(sa_apply_relu_bwd_kernel<decltype(r)::value>, dim3(fb_blocks(n4)), dim3(256), 0, (hipStream_t)stream, dout,
                           a, dgap, x0, dx, n4, HW, Cp, 1.f / HW);
    });
    return sc_check_launch("sa_apply_relu_bwd");
}

extern "C" int scouter_sa_apply_relu_bwd_f32(const float* dout, const float* a, const float* dgap, const float* x0, float* dx,
                                             int B, int HW, int Cp, void* stream) {
    return sa_apply_relu_bwd_launch(dout, a, dgap, x0, dx, B, HW, Cp, RULE_GRADIENT, stream);
}

extern "C" int scouter_sa_apply_relu_bwd_rule_f32(const float* dout, const float* a, const float* dgap, const float* x0, float* dx,
                                                  int B, int HW, int Cp, int rule, void* stream) {
    return sa_apply_relu_bwd_launch(dout, a, dgap, x0, dx, B, HW, Cp, rule, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// dx[b,iy,ix,c] = h[b,iy,ix,c] > 0 ? sum over the windows (oy, ox) that cover (iy, ix) and chose it, of dy[b,oy,ox,c] : +0
// The gather of the max-pool backward (bn_elem.hip) with the mask of the ReLU in front of the pool.  The windows of an input
// pixel are enumerated directly -- o in [ceil((t - k + 1) / stride), floor(t / stride)], t = i + pad -- and added in the order
// scouter_maxpool_bwd_f32 adds them for the same shape, so that the result is, bit for bit, that call followed by
// scouter_relu_bwd_f32: ascending (oy, ox) in the layout of its rows kernel (one workgroup row per input pixel row, threads along
// (ix, channel quad), stride 1 / 2 as a template argument: no division by a run-time stride) wherever that kernel runs, descending
// in a grid-stride kernel wherever its grid-stride kernel does.  RULE (relu_rule.h) acts on the gathered sum; the gather itself is
// the ordinary one under every rule, and rule 2 does not read h.
// ---------------------------------------------------------------------------------------------------------------
struct PoolBwdGeom { int B, H, W, C, Ho, Wo, k, stride, pad; };

__device__ __forceinline__ void pool_take(f32x4& acc, const float* __restrict__ dy, const unsigned char* __restrict__ arg, long o,
                                          int tap) {
    const uchar4 t = *(const uchar4*)(arg + o);
    const f32x4 d = *(const f32x4*)(dy + o);
    if (t.x == tap) acc[0] += d[0];
    if (t.y == tap) acc[1] += d[1];
    if (t.z == tap) acc[2] += d[2];
    if (t.w == tap) acc[3] += d[3];
}
template <int RULE>
__device__ __forceinline__ void pool_mask_store(f32x4 acc, const float* __restrict__ h, float* __restrict__ dx, long off) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (rule_reads_activation<RULE>) v = __builtin_nontemporal_load((const f32x4*)(h + off));
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = relu_rule<RULE>(acc[e], v[e]);
    *(f32x4*)(dx + off) = acc;
}

template <int S, int RULE>
__global__ __launch_bounds__(256) void maxpool_relu_bwd_rows_kernel(const float* __restrict__ dy,
                                                                    const unsigned char* __restrict__ arg,
                                                                    const float* __restrict__ h, float* __restrict__ dx,
                                                                    PoolBwdGeom g, float inv_c4n) {
    const int c4n = g.C / 4;
    const int xid = blockIdx.x * 256 + threadIdx.x;
    if (xid >= g.W * c4n) return;
    const int ix = (int)(((float)xid + 0.5f) * inv_c4n), cq = xid - ix * c4n;      // xid < 2^20: exact
    const int row = blockIdx.y, b = row / g.H, iy = row - b * g.H;
    const int ty = iy + g.pad, tx = ix + g.pad;
    const int oy_hi = min(ty / S, g.Ho - 1), ox_hi = min(tx / S, g.Wo - 1);
    const int oy_lo = ty - g.k + 1 <= 0 ? 0 : (ty - g.k + S) / S, ox_lo = tx - g.k + 1 <= 0 ? 0 : (tx - g.k + S) / S;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
        const int ky = ty - oy * S;
        for (int ox = ox_lo; ox <= ox_hi; ++ox)
            pool_take(acc, dy, arg, (((long)b * g.Ho + oy) * g.Wo + ox) * g.C + cq * 4, ky * g.k + (tx - ox * S));
    }
    pool_mask_store<RULE>(acc, h, dx, ((long)row * g.W + ix) * g.C + cq * 4);
}

template <int RULE>
__global__ __launch_bounds__(256) void maxpool_relu_bwd_grid_kernel(const float* __restrict__ dy,
                                                                    const unsigned char* __restrict__ arg,
                                                                    const float* __restrict__ h, float* __restrict__ dx,
                                                                    PoolBwdGeom g) {
    const int c4n = g.C / 4;
    const long n = (long)g.B * g.H * g.W * c4n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        long p = i / c4n;
        const int ix = (int)(p % g.W); p /= g.W;
        const int iy = (int)(p % g.H);
        const int b = (int)(p / g.H);
        const int ty = iy + g.pad, tx = ix + g.pad;
        const int oy_hi = min(ty / g.stride, g.Ho - 1), ox_hi = min(tx / g.stride, g.Wo - 1);
        const int oy_lo = ty - g.k + 1 <= 0 ? 0 : (ty - g.k + g.stride) / g.stride;
        const int ox_lo = tx - g.k + 1 <= 0 ? 0 : (tx - g.k + g.stride) / g.stride;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int oy = oy_hi; oy >= oy_lo; --oy) {                   // (ky ascending, as maxpool_bwd_kernel walks its taps)
            const int ky = ty - oy * g.stride;
            for (int ox = ox_hi; ox >= ox_lo; --ox)
                pool_take(acc, dy, arg, (((long)b * g.Ho + oy) * g.Wo + ox) * g.C + c, ky * g.k + (tx - ox * g.stride));
        }
        pool_mask_store<RULE>(acc, h, dx, i * 4);
    }
}

extern "C" int scouter_pool_out_size(int in, int k, int stride, int pad, int ceil_mode);

static int maxpool_relu_bwd_launch(const float* dy, const unsigned char* argmax, const float* h, float* dx, int B, int H, int W,
                                   int C, int k, int stride, int pad, int rule, void* stream) {
    SC_REQUIRE(dy && argmax && h && dx, "maxpool_relu_bwd: null pointer");
    SC_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && k > 0 && k <= 15 && stride > 0 && pad >= 0 && pad < k,
               "maxpool_relu_bwd: bad shape");
    const int Ho = scouter_pool_out_size(H, k, stride, pad, 0), Wo = scouter_pool_out_size(W, k, stride, pad, 0);
    SC_REQUIRE(Ho > 0 && Wo > 0, "maxpool_relu_bwd: the window does not fit the input");
    SC_REQUIRE_RULE(rule, "maxpool_relu_bwd");
    PoolBwdGeom g{B, H, W, C, Ho, Wo, k, stride, pad};
    hipStream_t st = (hipStream_t)stream;
    // (the rule of bn_elem.hip pool_bwd_rows_ok: where scouter_maxpool_bwd_f32 runs its rows kernel)
    const long xw = (long)W * (C / 4), rows = (long)B * H;
    const bool by_rows = (stride == 1 || stride == 2) && xw < (1 << 20) && rows <= 65535;
    ScProfScope prof(by_rows ? "maxpool_relu_bwd<rows>" : "maxpool_relu_bwd<grid>", st, 0,
                     (rule == RULE_DECONVNET ? 4.0 : 8.0) * (double)B * H * W * C + 5.0 * (double)B * Ho * Wo * C);
    rule_dispatch(rule, [&](auto r) {
        constexpr int RULE = decltype(r)::value;
        if (by_rows) {
            const dim3 grid((unsigned)((xw + 255) / 256), (unsigned)rows);
            const float inv = 1.0f / (float)(C / 4);
            if (stride == 1)
                hipLaunchKernelGGL((maxpool_relu_bwd_rows_kernel<1, RULE>), grid, dim3(256), 0, st, dy, argmax, h, dx, g, inv);
            else
                hipLaunchKernelGGL((maxpool_relu_bwd_rows_kernel<2, RULE>), grid, dim3(256), 0, st, dy, argmax, h, dx, g, inv);
        } else {
            hipLaunchKernelGGL(maxpool_relu_bwd_grid_kernel<RULE>, dim3(fb_blocks(rows * xw)), dim3(256), 0, st, dy, argmax, h, dx, g);
        }
    });
    return sc_check_launch("maxpool_relu_bwd");
}

extern "C" int scouter_maxpool_relu_bwd_f32(const float* dy, const unsigned char* argmax, const float* h, float* dx, int B,
                                            int H, int W, int C, int k, int stride, int pad, void* stream) {
    return maxpool_relu_bwd_launch(dy, argmax, h, dx, B, H, W, C, k, stride, pad, RULE_GRADIENT, stream);
}

extern "C" int scouter_maxpool_relu_bwd_rule_f32(const float* dy, const unsigned char* argmax, const float* h, float* dx, int B,
                                                 int H, int W, int C, int k, int stride, int pad, int rule, void* stream) {
    return maxpool_relu_bwd_launch(dy, argmax, h, dx, B, H, W, C, k, stride, pad, rule, stream);
}
