// The device expressions the attribution kernels share (gradcam.hip, gradcampp.hip, rise.hip, scorecam.hip, causal.hip,
// pathgrad.hip, fidelity.hip, extremal.hip, iba.hip, igos.hip, surrogate.hip, occlusion.hip, ablation.hip, layerattr.hip, gradshap.hip, guided.hip), each defined ONCE: where two kernels promise the same bits --
// heat_maps and cam_maps at the map's own size, resize_bilinear and the resize inside cam_maps and scorecam_ranges -- they call
// the same inlined function here on the same operands.  (The mask and the fma chain of the Score-CAM family have one file,
// scorecam.hip, and are defined there.)  Inlined functions and templates only: no kernel, no entry point, no state.
#pragma once
#include "common.h"

// the class-map kernels (gradcam_kernel, gradcampp_kernel): one workgroup per image, the channel weights in LDS
constexpr int AT_THREADS = 1024, AT_WAVES = AT_THREADS / 64, AT_MAX_C = 8192, AT_PART = AT_THREADS * 4;

typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------------------------
// Bilinear resize, align_corners = False: src = (dst + 0.5) scale - 0.5 clamped at 0 with scale = in / out, the lower index
// clamped to n - 1, the upper one min(lower + 1, n - 1).  Every index is clamped, so no value moves an address.

// source coordinate of destination index d: the lower neighbour, the upper one and its weight
__device__ __forceinline__ void at_source(int d, float scale, int n, int& i0, int& i1, float& t) {
    float s = fmaf((float)d + 0.5f, scale, -0.5f);
    s = fmaxf(s, 0.f);
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    t = s - (float)i0;
}

// the blend of the upper row's neighbours a0 / a1 and the lower row's b0 / b1 with column weight tx and row weight ty: three fmas
__device__ __forceinline__ float at_bilerp(float a0, float a1, float b0, float b1, float tx, float ty) {
    const float top = fmaf(tx, a1 - a0, a0), bot = fmaf(tx, b1 - b0, b0);
    return fmaf(ty, bot - top, top);
}

// ---------------------------------------------------------------------------------------------------------------------------
// minimum and maximum over a wave (butterfly; valid in every lane) ...
__device__ __forceinline__ void at_wave_minmax(float& lo, float& hi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
}

// ... and over a workgroup of WAVES waves, the waves in order through s_lo / s_hi [WAVES]; valid in every thread
template <int WAVES>
__device__ __forceinline__ void at_block_minmax(float& lo, float& hi, float* s_lo, float* s_hi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    at_wave_minmax(lo, hi);
    if (lane == 0) { s_lo[wv] = lo; s_hi[wv] = hi; }
    __syncthreads();
    lo = s_lo[0]; hi = s_hi[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); }
}

// sum of v over a workgroup of WAVES waves in a fixed order (lanes by butterfly, then the waves in order through s_part [WAVES]);
// the result is valid in thread 0.  Ends after one barrier: a second sum takes an s_part of its own.
template <int WAVES>
__device__ __forceinline__ double at_block_sum(double v, double* s_part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_part[wv] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < WAVES; ++i) t += s_part[i];
    return t;
}

// The two min-max scalings of a heat map as one affine map of v: ((v - lo) / span1 raised to lo2, minus lo2) / span2, to a byte.
// After the first scaling the minimum is exactly 0 and the maximum exactly 1, so the extrema of max(., min_level) are
// lo2 = max(0, min_level) and max(1, min_level).  A map that is constant at either step (or has a NaN / infinity in it) is flat.
struct AtHeatScale {
    float lo, span1, lo2, span2, min_level;
    bool flat;
    __device__ __forceinline__ AtHeatScale(float lo_, float hi, float min_level_) : lo(lo_), min_level(min_level_) {
        span1 = hi - lo;
        lo2 = fmaxf(0.f, min_level);
        span2 = fmaxf(1.f, min_level) - lo2;
        flat = !(span1 > 0.f) || !(span2 > 0.f);
    }
    __device__ __forceinline__ unsigned char byte(float v) const {
        float c = 0.f;
        if (!flat) {
            const float a = fmaxf((v - lo) / span1, min_level);
            c = fminf(fmaxf((a - lo2) / span2, 0.f), 1.f);
        }
        return (unsigned char)(int)(255.f * c);
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// The random streams of pathgrad.hip (noise_images), fidelity.hip (perturb_dots, uniform_images) and gradshap.hip, one copy for
// all.  The third counter word names the stream: 0 the normal stream, 1 the uniform stream of fidelity.hip, 2 the draws of
// gradshap.hip (gs_draw).
// Philox4x32-10 (Salmon et al., SC 2011): ten rounds, the key bumped between them
__device__ __forceinline__ void pg_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                          unsigned (&r)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// a random word -> (2 (r >> 9) + 1) 2^-24, exact in fp32 and inside (0, 1)
__device__ __forceinline__ float pg_uniform(unsigned r) { return (float)(2u * (r >> 9) + 1u) * 0x1p-24f; }

// one Box-Muller pair from two words, with the accurate library functions
__device__ __forceinline__ void pg_normal_pair(unsigned ra, unsigned rb, float& za, float& zb) {
    const float rad = sqrtf(-2.f * logf(pg_uniform(ra)));
    const float ang = 6.283185307179586f * pg_uniform(rb);
    za = rad * cosf(ang);
    zb = rad * sinf(ang);
}

// ---------------------------------------------------------------------------------------------------------------------------
// V = 1 or 4 consecutive elements with the widest access V allows (at most 16 bytes each); NT: streamed once, non-temporal
template <int V, bool NT = false>
__device__ __forceinline__ void at_load(const float* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        f32x4 t;
        if constexpr (NT) t = __builtin_nontemporal_load((const f32x4*)p);
        else t = *(const f32x4*)p;
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void at_load(const double* __restrict__ p, double (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = *p;
    } else {
#pragma unroll
        for (int k = 0; k < V; k += 2) {
            const f64x2 t = *(const f64x2*)(p + k);
            v[k] = t[0]; v[k + 1] = t[1];
        }
    }
}
template <int V>
__device__ __forceinline__ void at_store(float* __restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
    else *p = v[0];
}
template <int V>
__device__ __forceinline__ void at_store(double* __restrict__ p, const double (&v)[V]) {
    if constexpr (V == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int k = 0; k < V; k += 2) *(f64x2*)(p + k) = f64x2{v[k], v[k + 1]};
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The two passes of a class-map kernel, for a workgroup of AT_THREADS threads.
//
// Per column c: dst[c] = (D) finish(sum_p term(p, c)), term formed by `add(p, q, s, a)` for the V channels of column group q
// onto the running sums a, with s = the V values src[V q ..] of a per-channel LDS array (null: zeros).  The column groups are
// spread over the threads; when there are fewer of them than threads the positions are dealt to G = threads / groups groups,
// whose partial sums meet in part [AT_PART] and are added in group order.  Ends in a barrier.
template <int V, typename T, typename D, typename Add, typename Finish>
__device__ __forceinline__ void at_column_sums(Add add, Finish finish, const T* __restrict__ src, D* __restrict__ dst,
                                               T* __restrict__ part, int N, int C) {
    const int tid = threadIdx.x, cols = C / V;                // (V == 4: C is a multiple of 4)
    if (cols >= AT_THREADS) {
        for (int q = tid; q < cols; q += AT_THREADS) {
            T a[V], s[V];
#pragma unroll
            for (int k = 0; k < V; ++k) { a[k] = (T)0; s[k] = src ? src[V * q + k] : (T)0; }
#pragma unroll 4
            for (int p = 0; p < N; ++p) add(p, q, s, a);
#pragma unroll
            for (int k = 0; k < V; ++k) dst[V * q + k] = (D)finish(a[k]);
        }
    } else {
        int G = AT_THREADS / cols;
        if (G > N) G = N;
        const int g = tid / cols, q = tid - g * cols;
        if (g < G) {
            T a[V], s[V];
#pragma unroll
            for (int k = 0; k < V; ++k) { a[k] = (T)0; s[k] = src ? src[V * q + k] : (T)0; }
#pragma unroll 4
            for (int p = g; p < N; p += G) add(p, q, s, a);
#pragma unroll
            for (int k = 0; k < V; ++k) part[g * C + V * q + k] = a[k];          // (G * C <= AT_THREADS * V = AT_PART)
        }
        __syncthreads();
        for (int c = tid; c < C; c += AT_THREADS) {
            T a = part[c];
            for (int j = 1; j < G; ++j) a += part[j * C + c];
            dst[c] = (D)finish(a);
        }
    }
    __syncthreads();
}

// out[p] = sum_c s_w[c] ft[p][c] (relu: clamped at 0), one wave per position: a lane takes every 64th of the cols = C / V column
// groups, the 64 partial sums meet in a butterfly.  s_w is the LDS array [C] a column-sum pass left behind.
template <bool VEC>
__device__ __forceinline__ void at_contract_positions(const float* __restrict__ ft, const float* __restrict__ s_w,
                                                      float* __restrict__ o, int N, int C, int cols, int relu) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int p = wv; p < N; p += AT_WAVES) {
        const float* __restrict__ row = ft + (long)p * C;
        float a = 0.f;
        for (int q = lane; q < cols; q += 64) {
            if constexpr (VEC) {
                const f32x4 v = *(const f32x4*)(row + 4 * q);
                const f32x4 w = *(const f32x4*)(s_w + 4 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) a = fmaf(v[k], w[k], a);
            } else {
                a = fmaf(row[q], s_w[q], a);
            }
        }
        a = wave_sum(a);
        if (lane == 0) o[p] = relu ? fmaxf(a, 0.f) : a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// One mask value per pixel times every image channel: out[c][p ..] = image[c][p ..] m, V = 1 or 4 pixels of a row from flat
// index p (VEC: 16-byte loads and stores).
template <bool VEC>
__device__ __forceinline__ void at_scale_channels(const float* __restrict__ image, float* __restrict__ o, long plane, long p,
                                                  int Cin, const float (&m)[VEC ? 4 : 1]) {
    for (int c = 0; c < Cin; ++c) {
        if constexpr (VEC) {
            f32x4 v = *(const f32x4*)(image + c * plane + p);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] *= m[k];
            *(f32x4*)(o + c * plane + p) = v;
        } else {
            o[c * plane + p] = image[c * plane + p] * m[0];
        }
    }
}

// The launch geometry of a kernel that walks an H x W plane 1 or 4 pixels per thread: vec when W is a multiple of 4 and no
// pointer (their bits or-ed) has a low address bit set, items = the threads' work items, tiles = the grid's y extent (<= 65535;
// the kernels stride over the rest).
struct AtPixelGrid {
    bool vec;
    long items;
    unsigned tiles;
};
static inline AtPixelGrid at_pixel_grid(int H, int W, int threads, uintptr_t pointer_bits) {
    AtPixelGrid g;
    g.vec = W % 4 == 0 && (pointer_bits & 15) == 0;
    g.items = (long)H * (g.vec ? W / 4 : W);
    const long tiles = (g.items + threads - 1) / threads;
    g.tiles = (unsigned)(tiles > 65535 ? 65535 : tiles);
    return g;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The end the class-tiled kernels share (rise_accumulate_kernel, sscam_contract_kernel, ablation_contract_kernel):
// acc[k0 + k][p] = a[k] for the kt classes a thread holds in registers for element p of the plane
template <int KT>
__device__ __forceinline__ void at_store_acc(float* __restrict__ acc, long plane, long p, int k0, int kt, const float (&a)[KT]) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < kt) acc[(long)(k0 + k) * plane + p] = a[k];
}

// The step the class-tiled kernels share (rise_accumulate_kernel, sscam_contract_kernel, ablation_contract_kernel): one value v
// of the plane's element times the KT staged weights w [KT] of a term, one fma per class onto the accumulators
template <int KT>
__device__ __forceinline__ void at_fma_tile(const float* __restrict__ w, float v, float (&a)[KT]) {
#pragma unroll
    for (int k = 0; k < KT; ++k) a[k] = fmaf(w[k], v, a[k]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Extremal perturbation (extremal.hip): what its kernels must agree on bit for bit.  The smooth-max upsampler's window and
// kernel values -- extremal_mask forms them, extremal_step differentiates them -- and the knot of the blur pyramid, which
// extremal_blend uses and extremal_mask_grad recomputes.
constexpr float EX_BETA = 20.f;                 // the sharpness of the smooth max

// the window's radius in cells: a pixel sees the (2 r + 1)^2 cells around its own
static inline int ex_radius(int step, float sigma) { return 1 + (int)ceil((double)sigma / (double)step); }

// k(|u - centre| / sigma), k(z) = exp(-2 max(z - 0.5, 0)^2), for the pixel at (ym, xm) inside its own cell and the cell (a, b)
// cells away from it: u - centre = (ym - a step - (step - 1) / 2, xm - b step - (step - 1) / 2), half-integers that are exact
__device__ __forceinline__ float ex_kernel_value(int ym, int xm, int a, int b, int step, float sigma) {
    const float half = 0.5f * (float)(step - 1);
    const float dy = (float)(ym - a * step) - half, dx = (float)(xm - b * step) - half;
    const float d = fmaxf(sqrtf(fmaf(dy, dy, dx * dx)) / sigma - 0.5f, 0.f);
    return expf(-2.f * d * d);
}

// tab[((ym step + xm) D + a + r) D + b + r] = ex_kernel_value(ym, xm, a, b), D = 2 r + 1: step^2 D^2 floats, once per workgroup
// (the caller's barrier follows)
template <int THREADS>
__device__ __forceinline__ void ex_fill_table(float* __restrict__ tab, int step, int r, float sigma) {
    const int D = 2 * r + 1, DD = D * D, T = step * step * DD;
    for (int t = threadIdx.x; t < T; t += THREADS) {
        const int pm = t / DD, ab = t - pm * DD, ia = ab / D, ib = ab - ia * D;
        tab[t] = ex_kernel_value(pm / step, pm % step, ia - r, ib - r, step, sigma);
    }
}

// the piece of the blur pyramid a mask value m selects: m' = m (variant 0, preserve) or 1 - m (variant 1, delete),
// t = m' (L - 1) clamped to [0, L - 1] (a NaN goes to 0, so no value moves an address), k = min(floor(t), L - 2), w = t - k:
// the right-hand piece at an interior knot, the last piece with w = 1 at m' = 1
__device__ __forceinline__ void ex_knot(float m, int variant, int L, int& k, float& w) {
    const float mp = variant ? 1.f - m : m;
    const float t = fminf(fmaxf(mp * (float)(L - 1), 0.f), (float)(L - 1));
    k = min((int)t, L - 2);
    w = t - (float)k;
}

// (1 - w) p0 + w p1, exact at both ends: p0 at w = 0 and p1 at w = 1
__device__ __forceinline__ float ex_mix(float p0, float p1, float w) { return fmaf(w, p1, (1.f - w) * p0); }

// ---------------------------------------------------------------------------------------------------------------------------
// Information-bottleneck attribution (iba.hip): what iba_sample and iba_step must agree on bit for bit.  The smoothing window's
// values, the reflecting index map with its adjoint, and the counter layout of the noise -- the stream of noise_images.
constexpr int IB_MAX_R = 6, IB_MAX_D = 2 * IB_MAX_R + 1;       // sigma up to 3.25

// the window's radius: round(2 sigma) to even at a tie, as Python's round; no smoothing (radius 0) for sigma <= 0
static inline int ib_radius(float sigma) { return sigma > 0.f ? (int)nearbyint(2.0 * (double)sigma) : 0; }

// w[a D + b] = exp(-((a - r)^2 + (b - r)^2) / (2 sigma^2)) / the sum of all of them, D = 2 r + 1: formed in fp64 and rounded once;
// the one value 1 at radius 0
struct IbWindow {
    int r;
    float w[IB_MAX_D * IB_MAX_D];
};
static inline void ib_window(float sigma, IbWindow& win) {      // (the caller has refused a radius above IB_MAX_R)
    const int r = win.r = ib_radius(sigma), D = 2 * r + 1;
    double g[IB_MAX_D], tot = 0.0;
    for (int d = 0; d < D; ++d) {
        g[d] = r ? exp(-(double)((d - r) * (d - r)) / (2.0 * (double)sigma * (double)sigma)) : 1.0;
        tot += g[d];
    }
    for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) win.w[a * D + b] = (float)(g[a] * g[b] / (tot * tot));
}

// index i of an axis of n cells padded by reflection without the edge (ReflectionPad2d), -(n - 1) <= i <= 2 (n - 1)
__device__ __forceinline__ int ib_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// the adjoint of ib_reflect: the padded indices u in [-r, n - 1 + r] that map to cell c -- c itself, its mirror below 0 and its
// mirror above n - 1 -- into u[3]; returns how many (r <= n - 1: a cell is mirrored at most once per side)
__device__ __forceinline__ int ib_sources(int c, int n, int r, int (&u)[3]) {
    int cnt = 1;
    u[0] = c; u[1] = c; u[2] = c;
    if (c > 0 && c <= r) u[cnt++] = -c;
    if (c < n - 1 && n - 1 - c <= r) u[cnt++] = 2 * (n - 1) - c;
    return cnt;
}

// eps of the V = 4 elements e .. e + 3 (e a multiple of 4) or of the one element e of sample `sample`: the Philox words of the
// counter (e / 4, sample, 0, 0) through two Box-Muller pairs, as noise_images_kernel forms them
template <int V>
__device__ __forceinline__ void ib_noise(long e, unsigned sample, unsigned seed_lo, unsigned seed_hi, float (&z)[V]) {
    unsigned r[4];
    pg_philox((unsigned)(e >> 2), sample, 0u, 0u, seed_lo, seed_hi, r);
    if constexpr (V == 4) {
        pg_normal_pair(r[0], r[1], z[0], z[1]);
        pg_normal_pair(r[2], r[3], z[2], z[3]);
    } else {
        const int i = (int)(e & 3);
        float za, zb;
        pg_normal_pair((i & 2) ? r[2] : r[0], (i & 2) ? r[3] : r[1], za, zb);
        z[0] = (i & 1) ? zb : za;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// I-GOS (igos.hip): what its kernels must agree on bit for bit.  The align-corners upsampler (torch.nn.UpsamplingBilinear2d) --
// igos_upsample, igos_path_images and igos_trial_images form it, igos_mask_grad gathers its adjoint through the same source
// coordinates -- and the candidate cell of the line search, which igos_trial_images evaluates and igos_step stores.

// the scale of an axis of n_in cells upsampled to n_out >= 2 pixels: the ends of the two grids coincide
static inline float ig_scale(int n_in, int n_out) { return (float)(n_in - 1) / (float)(n_out - 1); }

// source coordinate of destination index d, align_corners = True: s = d scale, the lower index clamped to n - 1, the upper one
// min(lower + 1, n - 1), t = s - lower.  Every index is clamped, so no value moves an address.  s is the ROUNDED product:
// contraction is switched off here, or the compiler fuses the product into the difference and t = fma(d, scale, -lower) carries
// the bits the rounding of s drops (seen on gfx950: t off by up to 6e-8 at 3 cells -> 13 pixels).
__device__ __forceinline__ void ig_source(int d, float scale, int n, int& i0, int& i1, float& t) {
#pragma clang fp contract(off)
    const float s = (float)d * scale;
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    t = s - (float)i0;
}

// the cell the line search tries at step size `step` along -dm: clamp(p - step dm, 0, 1); a NaN goes to 0
__device__ __forceinline__ float ig_candidate(float p, float dm, float step) {
    return fminf(fmaxf(fmaf(-step, dm, p), 0.f), 1.f);
}

// the upsampled value of a pixel from its four cells, cell(i) the value of cell i of the row-major hm x wm grid
template <typename Cell>
__device__ __forceinline__ float ig_upsample_at(Cell cell, int wm, int y0, int y1, float ty, int x0, int x1, float tx) {
    return at_bilerp(cell(y0 * wm + x0), cell(y0 * wm + x1), cell(y1 * wm + x0), cell(y1 * wm + x1), tx, ty);
}

