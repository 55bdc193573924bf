// Extremal perturbation (Fong, Patrick, Vedaldi, ICCV 2019; torchray.attribution.extremal_perturbation, what the reference's
// torchcam_vis.py runs after RISE): the mask side of one optimisation step (tools/attribution.py extremal_perturbation).  n
// coarse masks pmask [n][hm][wm] in [0, 1] on a grid of `step` pixels, hm = ceil(H / step), wm = ceil(W / step), one image's
// blur pyramid P [L][C][H][W].  Five kernels, one launch each, no atomics, every cross-thread sum in one fixed order: two calls
// give the same bits, and a mask's values do not depend on the other masks of the call.
//
// extremal_mask_kernel: the smooth-max upsampling.  Pixel u = (y, x) sees the D^2 = (2 r + 1)^2 cells (y / step + a,
//   x / step + b), a, b in [-r, r], r = 1 + ceil(sigma / step) (ex_radius); cell c takes part with v_c = k_c p_c,
//   k_c = ex_kernel_value (attr_common.h), 0 for a cell outside the grid; m(u) = sum_c v_c e_c / sum_c e_c with
//   e_c = expf(EX_BETA (v_c - vmax)), vmax the window's maximum.  k depends on (y mod step, x mod step, a, b) alone: the
//   step^2 D^2 values are formed once per workgroup into LDS (ex_fill_table; 15.5 KB at step 7, sigma 21), a workgroup then
//   strides over the pixels.  Two passes over the window in (a, b) order: the maximum, then den += e, num = fma(v, e, num).  The
//   softmax statistics (vmax, den) of every pixel go to `stats` [n][H W][2] when it is given: extremal_step reads them back
//   instead of walking the window again.
// extremal_blend_kernel: out[j][ch][y][x] = ex_mix(P[k][ch][q], P[k + 1][ch][q], w), (k, w) = ex_knot(mask[j][q]) and q = (y, x),
//   or (y, W - 1 - x) when `flip` is set (the mirrored image).  The 16-byte form (W a multiple of 4, every pointer 16-byte
//   aligned; at_pixel_grid) takes four pixels of a row per thread: the mask by one 16-byte load, the output by 16-byte stores,
//   the two pyramid levels by 16-byte loads when the four pixels share their piece k (a smooth mask: nearly always) and one
//   element at a time otherwise; the one-element form takes one pixel.  The same expression on the same operands: equal bits.
// extremal_seed_kernel: one thread per element of seed [n][n_out]: -+expf(logp[j][cols[j]]) in column cols[j] (- for preserve,
//   + for delete: d loss / d log-probability), 0 elsewhere; the thread of column 0 also writes rewards[it][j] = that expf.
// extremal_mask_grad_kernel: dmask[j][q] = fma(+-(L - 1), sum_ch dx[j][ch][q'] (P[k + 1] - P[k])[ch][q], c2 (m(q) - tau(q))),
//   the sum by one fma per channel in ascending ch, (k, .) = ex_knot(mask[j][q]) -- the piece extremal_blend used, from the same
//   expression -- q' = q mirrored when `flip` is set, tau(q) = 1 where ranks[j][q] < targets[j], c2 = 2 lam / (H W) formed in
//   fp64 on the host and rounded once.  One pixel per thread.
// extremal_step_kernel: per cell c of mask j the gather g = sum_u dmask(u) k_uc w_uc (1 + EX_BETA (v_uc - m(u))) over the at
//   most (D step)^2 pixels u that see the cell, v_uc = k_uc p_c, w_uc = expf(EX_BETA (v_uc - vmax_u)) / den_u from `stats`, then
//   buf = g (first) or fma(mu, buf, (1 - mu) g) and p = clamp(fma(-lr, buf, p), 0, 1), IN PLACE.  One wave per cell (a workgroup
//   of four waves takes EX_STEP_CELLS cells per wave, one k table for all of them): a lane adds its pixels
//   t = lane, lane + 64, ... of the cell's (D step)^2 window in ascending t by one fma each, then a butterfly over the wave.
//   The in-place write is free of races: the terms of cell c read p_c -- its own cell, which only this wave writes, after its
//   sum -- and per-pixel quantities (mask, dmask, stats) that no thread of the launch writes; no other cell's p enters.
#include "attr_common.h"

constexpr int EX_THREADS = 256, EX_WAVES = EX_THREADS / 64;
constexpr int EX_MASK_PIXELS = 4;                 // pixels per thread of extremal_mask (the k table serves 1024 pixels)
constexpr int EX_STEP_CELLS = 4;                  // cells per wave of extremal_step (the k table serves 16 cells)
constexpr int EX_MAX_TABLE = 16384;               // floats of the k table: 64 KB of LDS

struct ExGeometry {
    int hm, wm, r, table;
};

// the grid, the window and the k table of (H, W, step, sigma), with the refusals every kernel that uses them shares
static int ex_geometry(const char* what, int H, int W, int step, float sigma, ExGeometry& g) {
    SC_REQUIRE(H > 0 && W > 0 && step > 0, "%s: bad arguments (H %d, W %d, step %d: each must be at least 1)", what, H, W, step);
    SC_REQUIRE(sigma > 0.f && sigma <= 3.0e38f, "%s: sigma = %g (it must be positive and finite)", what, (double)sigma);
    SC_UNSUPPORTED((long)H * W < (1L << 31), "%s: a mask of %d x %d pixels is past the 32-bit offsets", what, H, W);
    SC_UNSUPPORTED((double)sigma / step <= 64.0, "%s: sigma / step = %g (at most 64)", what, (double)sigma / step);
    g.hm = (H + step - 1) / step;
    g.wm = (W + step - 1) / step;
    g.r = ex_radius(step, sigma);
    const long D = 2L * g.r + 1, table = (long)step * step * D * D;
    SC_UNSUPPORTED(table <= EX_MAX_TABLE, "%s: step %d and sigma %g need a kernel table of %ld floats (at most %d)", what, step,
                   (double)sigma, table, EX_MAX_TABLE);
    g.table = (int)table;
    return SC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_THREADS) void extremal_mask_kernel(const float* __restrict__ pmask, float* __restrict__ out,
                                                                   float* __restrict__ stats, int H, int W, int hm, int wm,
                                                                   int step, int r, float sigma) {
    extern __shared__ __attribute__((aligned(16))) float s_tab[];
    ex_fill_table<EX_THREADS>(s_tab, step, r, sigma);
    __syncthreads();
    const int D = 2 * r + 1;
    const long plane = (long)H * W;
    const float* __restrict__ pm = pmask + (long)blockIdx.y * hm * wm;
    for (long p = (long)blockIdx.x * EX_THREADS + threadIdx.x; p < plane; p += (long)gridDim.x * EX_THREADS) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const int cy = y / step, cx = x / step;
        const float* __restrict__ tab = s_tab + ((y - cy * step) * step + (x - cx * step)) * D * D;
        float vmax = 0.f;                                                     // (the first cell replaces it)
        for (int ia = 0; ia < D; ++ia) {
            const int ci = cy + ia - r;
            const bool row = ci >= 0 && ci < hm;
            for (int ib = 0; ib < D; ++ib) {
                const int cj = cx + ib - r;
                const float v = row && cj >= 0 && cj < wm ? tab[ia * D + ib] * pm[ci * wm + cj] : 0.f;
                vmax = (ia | ib) == 0 ? v : fmaxf(vmax, v);
            }
        }
        float num = 0.f, den = 0.f;
        for (int ia = 0; ia < D; ++ia) {
            const int ci = cy + ia - r;
            const bool row = ci >= 0 && ci < hm;
            for (int ib = 0; ib < D; ++ib) {
                const int cj = cx + ib - r;
                const float v = row && cj >= 0 && cj < wm ? tab[ia * D + ib] * pm[ci * wm + cj] : 0.f;
                const float e = expf(EX_BETA * (v - vmax));
                den += e;
                num = fmaf(v, e, num);
            }
        }
        const long q = (long)blockIdx.y * plane + p;
        out[q] = num / den;
        if (stats) {
            stats[2 * q] = vmax;
            stats[2 * q + 1] = den;
        }
    }
}

extern "C" int scouter_extremal_mask_f32(const float* pmask, float* out, float* stats, int n, int H, int W, int step, float sigma,
                                         void* stream) {
    SC_REQUIRE(pmask && out, "extremal_mask: null pointer (pmask %p, out %p)", (const void*)pmask, (void*)out);
    SC_REQUIRE(n > 0, "extremal_mask: n = %d (at least 1)", n);
    ExGeometry g;
    if (int rc = ex_geometry("extremal_mask", H, W, step, sigma, g)) return rc;
    SC_REQUIRE((((uintptr_t)pmask | (uintptr_t)out | (uintptr_t)stats) & 3) == 0,
               "extremal_mask: misaligned pointer (pmask, out and stats must be 4-byte aligned)");
    SC_UNSUPPORTED(n <= 65535, "extremal_mask: n = %d masks (at most 65535 per call)", n);
    hipStream_t st = (hipStream_t)stream;
    const long plane = (long)H * W;
    const double D2 = (2.0 * g.r + 1.0) * (2.0 * g.r + 1.0);
    ScProfScope prof("extremal_mask", st, 30.0 * D2 * n * (double)plane, 4.0 * n * ((stats ? 3.0 : 1.0) * plane + (double)g.hm * g.wm));
    const dim3 grid((unsigned)sc_cdiv(plane, (long)EX_THREADS * EX_MASK_PIXELS), (unsigned)n);
    hipLaunchKernelGGL(extremal_mask_kernel, grid, dim3(EX_THREADS), (size_t)g.table * sizeof(float), st, pmask, out, stats, H, W,
                       g.hm, g.wm, step, g.r, sigma);
    return sc_check_launch("extremal_mask");
}

// ---------------------------------------------------------------------------------------------------------------------------
static int ex_check_pyramid(const char* what, int n, int L, int C, int H, int W, int variant, int flip) {
    SC_REQUIRE(n > 0 && C > 0 && H > 0 && W > 0, "%s: bad arguments (n %d, C %d, H %d, W %d: each must be at least 1)", what, n, C,
               H, W);
    SC_REQUIRE(L >= 2, "%s: L = %d (a pyramid has at least 2 levels)", what, L);
    SC_REQUIRE((variant == 0 || variant == 1) && (flip == 0 || flip == 1),
               "%s: variant = %d, flip = %d (variant 0: preserve, 1: delete; flip 0 or 1)", what, variant, flip);
    SC_UNSUPPORTED((double)L * C * H * W < 2147483648.0 && (double)n * C * H * W < 2147483648.0,
                   "%s: %d levels or %d images of %d x %d x %d elements are past the 32-bit offsets", what, L, n, C, H, W);
    SC_UNSUPPORTED(n <= 65535, "%s: n = %d masks (at most 65535 per call)", what, n);
    return SC_OK;
}

template <bool VEC>
__global__ __launch_bounds__(EX_THREADS) void extremal_blend_kernel(const float* __restrict__ pyramid,
                                                                    const float* __restrict__ mask, float* __restrict__ out, int L,
                                                                    int C, int H, int W, int variant, int flip) {
    const long plane = (long)H * W;
    const float* __restrict__ mk = mask + (long)blockIdx.x * plane;
    float* __restrict__ o = out + (long)blockIdx.x * C * plane;
    constexpr int V = VEC ? 4 : 1;
    const int wq = W / V;                                                     // (VEC: W is a multiple of 4)
    const long items = (long)H * wq;
    for (long i = (long)blockIdx.y * EX_THREADS + threadIdx.x; i < items; i += (long)gridDim.y * EX_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        const long dst = (long)y * W + x;
        // the V source pixels, in ascending address: [src, src + V); output pixel x + e reads source pixel e (or V - 1 - e)
        const long src = flip ? (long)y * W + (W - V - x) : dst;
        if constexpr (VEC) {
            const f32x4 m4 = *(const f32x4*)(mk + src);
            int k[4];
            float w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) ex_knot(m4[e], variant, L, k[e], w[e]);
            const bool same = k[0] == k[1] && k[0] == k[2] && k[0] == k[3];
            for (int c = 0; c < C; ++c) {
                f32x4 v;
                if (same) {
                    const f32x4 p0 = *(const f32x4*)(pyramid + ((long)k[0] * C + c) * plane + src);
                    const f32x4 p1 = *(const f32x4*)(pyramid + ((long)(k[0] + 1) * C + c) * plane + src);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = ex_mix(p0[e], p1[e], w[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float* __restrict__ pp = pyramid + ((long)k[e] * C + c) * plane + src + e;
                        v[e] = ex_mix(pp[0], pp[(long)C * plane], w[e]);
                    }
                }
                if (flip) v = f32x4{v[3], v[2], v[1], v[0]};
                *(f32x4*)(o + c * plane + dst) = v;
            }
        } else {
            int k;
            float w;
            ex_knot(mk[src], variant, L, k, w);
            for (int c = 0; c < C; ++c) {
                const float* __restrict__ pp = pyramid + ((long)k * C + c) * plane + src;
                o[c * plane + dst] = ex_mix(pp[0], pp[(long)C * plane], w);
            }
        }
    }
}

extern "C" int scouter_extremal_blend_f32(const float* pyramid, const float* mask, float* out, int n, int L, int C, int H, int W,
                                          int variant, int flip, void* stream) {
    SC_REQUIRE(pyramid && mask && out, "extremal_blend: null pointer (pyramid %p, mask %p, out %p)", (const void*)pyramid,
               (const void*)mask, (void*)out);
    if (int rc = ex_check_pyramid("extremal_blend", n, L, C, H, W, variant, flip)) return rc;
    SC_REQUIRE((((uintptr_t)pyramid | (uintptr_t)mask | (uintptr_t)out) & 3) == 0,
               "extremal_blend: misaligned pointer (pyramid, mask and out must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, EX_THREADS, (uintptr_t)pyramid | (uintptr_t)mask | (uintptr_t)out);
    const double elems = (double)n * C * H * W;
    ScProfScope prof("extremal_blend", st, 4.0 * elems, 4.0 * (3.0 * elems + (double)n * H * W));
    const dim3 grid((unsigned)n, px.tiles);
    if (px.vec)
        hipLaunchKernelGGL(extremal_blend_kernel<true>, grid, dim3(EX_THREADS), 0, st, pyramid, mask, out, L, C, H, W, variant,
                           flip);
    else
        hipLaunchKernelGGL(extremal_blend_kernel<false>, grid, dim3(EX_THREADS), 0, st, pyramid, mask, out, L, C, H, W, variant,
                           flip);
    return sc_check_launch("extremal_blend");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_THREADS) void extremal_seed_kernel(const float* __restrict__ logp, const int* __restrict__ cols,
                                                                   float* __restrict__ seed, float* __restrict__ rewards, int n,
                                                                   int n_out, int it, int variant) {
    const long i = (long)blockIdx.x * EX_THREADS + threadIdx.x;
    if (i >= (long)n * n_out) return;
    const int j = (int)(i / n_out), c = (int)(i - (long)j * n_out);
    const int col = min(max(cols[j], 0), n_out - 1);                          // (the host refuses an index outside)
    float v = 0.f;
    if (c == col || c == 0) {
        const float p = expf(logp[(long)j * n_out + col]);
        if (c == col) v = variant ? p : -p;
        if (c == 0) rewards[(long)it * n + j] = p;
    }
    seed[i] = v;
}

extern "C" int scouter_extremal_seed_f32(const float* logp, const int* cols, float* seed, float* rewards, int n, int n_out,
                                         int n_iters, int it, int variant, void* stream) {
    SC_REQUIRE(logp && cols && seed && rewards, "extremal_seed: null pointer (logp %p, cols %p, seed %p, rewards %p)",
               (const void*)logp, (const void*)cols, (void*)seed, (void*)rewards);
    SC_REQUIRE(n > 0 && n_out > 0, "extremal_seed: bad arguments (n %d, n_out %d: each must be at least 1)", n, n_out);
    SC_REQUIRE(it >= 0 && it < n_iters, "extremal_seed: iteration %d lies outside [0, n_iters = %d)", it, n_iters);
    SC_REQUIRE(variant == 0 || variant == 1, "extremal_seed: variant = %d (0: preserve, 1: delete)", variant);
    SC_REQUIRE((((uintptr_t)logp | (uintptr_t)cols | (uintptr_t)seed | (uintptr_t)rewards) & 3) == 0,
               "extremal_seed: misaligned pointer (logp, cols, seed and rewards must be 4-byte aligned)");
    SC_UNSUPPORTED((long)n * n_out < (1L << 31) && (long)n_iters * n < (1L << 31),
                   "extremal_seed: %d rows of %d outputs or %d iterations are past the 32-bit offsets", n, n_out, n_iters);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("extremal_seed", st, 10.0 * n, 4.0 * (n * (double)n_out + 3.0 * n));
    hipLaunchKernelGGL(extremal_seed_kernel, dim3((unsigned)sc_cdiv((long)n * n_out, EX_THREADS)), dim3(EX_THREADS), 0, st, logp,
                       cols, seed, rewards, n, n_out, it, variant);
    return sc_check_launch("extremal_seed");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_THREADS) void extremal_mask_grad_kernel(const float* __restrict__ pyramid,
                                                                        const float* __restrict__ mask, const float* __restrict__ dx,
                                                                        const int* __restrict__ ranks, const int* __restrict__ targets,
                                                                        float* __restrict__ dmask, float c2, int L, int C, int H,
                                                                        int W, int variant, int flip) {
    const long plane = (long)H * W;
    const int j = blockIdx.x;
    const float* __restrict__ g = dx + (long)j * C * plane;
    const int area = targets[j];
    const float scale = variant ? -(float)(L - 1) : (float)(L - 1);
    for (long q = (long)blockIdx.y * EX_THREADS + threadIdx.x; q < plane; q += (long)gridDim.y * EX_THREADS) {
        const int y = (int)(q / W), x = (int)(q - (long)y * W);
        const long qf = flip ? (long)y * W + (W - 1 - x) : q;
        const float m = mask[(long)j * plane + q];
        int k;
        float w;
        ex_knot(m, variant, L, k, w);
        float acc = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ pp = pyramid + ((long)k * C + c) * plane + q;
            acc = fmaf(g[c * plane + qf], pp[(long)C * plane] - pp[0], acc);
        }
        const float tau = ranks[(long)j * plane + q] < area ? 1.f : 0.f;
        dmask[(long)j * plane + q] = fmaf(scale, acc, c2 * (m - tau));
    }
}

extern "C" int scouter_extremal_mask_grad_f32(const float* pyramid, const float* mask, const float* dx, const int* ranks,
                                              const int* targets, float* dmask, float lam, int n, int L, int C, int H, int W,
                                              int variant, int flip, void* stream) {
    SC_REQUIRE(pyramid && mask && dx && ranks && targets && dmask,
               "extremal_mask_grad: null pointer (pyramid %p, mask %p, dx %p, ranks %p, targets %p, dmask %p)", (const void*)pyramid,
               (const void*)mask, (const void*)dx, (const void*)ranks, (const void*)targets, (void*)dmask);
    if (int rc = ex_check_pyramid("extremal_mask_grad", n, L, C, H, W, variant, flip)) return rc;
    SC_REQUIRE(lam >= 0.f && lam <= 3.0e38f, "extremal_mask_grad: lam = %g (it must be finite and not negative)", (double)lam);
    SC_REQUIRE((((uintptr_t)pyramid | (uintptr_t)mask | (uintptr_t)dx | (uintptr_t)ranks | (uintptr_t)targets | (uintptr_t)dmask) & 3)
                   == 0, "extremal_mask_grad: misaligned pointer (every array must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, EX_THREADS, 1);                // (one pixel per thread)
    const double pix = (double)n * H * W;
    ScProfScope prof("extremal_mask_grad", st, (3.0 * C + 8.0) * pix, 4.0 * (3.0 * C + 3.0) * pix);
    const float c2 = (float)(2.0 * (double)lam / ((double)H * W));
    hipLaunchKernelGGL(extremal_mask_grad_kernel, dim3((unsigned)n, px.tiles), dim3(EX_THREADS), 0, st, pyramid, mask, dx, ranks,
                       targets, dmask, c2, L, C, H, W, variant, flip);
    return sc_check_launch("extremal_mask_grad");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_THREADS) void extremal_step_kernel(float* __restrict__ pmask, float* __restrict__ mom,
                                                                   const float* __restrict__ mask, const float* __restrict__ dmask,
                                                                   const float* __restrict__ stats, long cells_total, int H, int W,
                                                                   int hm, int wm, int step, int r, float sigma, float lr, float mu,
                                                                   int first) {
    extern __shared__ __attribute__((aligned(16))) float s_tab[];
    ex_fill_table<EX_THREADS>(s_tab, step, r, sigma);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int D = 2 * r + 1, side = D * step, cells = hm * wm;
    const long plane = (long)H * W;
    for (int i = 0; i < EX_STEP_CELLS; ++i) {
        const long c = ((long)blockIdx.x * EX_WAVES + wv) * EX_STEP_CELLS + i;   // (uniform over the wave)
        if (c >= cells_total) break;
        const int j = (int)(c / cells), cc = (int)(c - (long)j * cells);
        const int ci = cc / wm, cj = cc - ci * wm;
        const int y0 = (ci - r) * step, x0 = (cj - r) * step;                 // the first pixel of the window that sees the cell
        const float pc = pmask[c];
        float g = 0.f;
        for (int t = lane; t < side * side; t += 64) {
            const int ly = t / side, lx = t - ly * side;
            const int y = y0 + ly, x = x0 + lx;
            if (y < 0 || y >= H || x < 0 || x >= W) continue;
            // the pixel's own cell is (ci - r + ly / step, cj - r + lx / step): this cell is (a, b) = (r - ly / step, r - lx / step)
            // away from it, entry (a + r, b + r) of the pixel's table
            const int cy = ly / step, cx = lx / step;
            const float kk = s_tab[(((ly - cy * step) * step + (lx - cx * step)) * D + 2 * r - cy) * D + 2 * r - cx];
            const long q = (long)j * plane + (long)y * W + x;
            const float v = kk * pc;
            const float w = expf(EX_BETA * (v - stats[2 * q])) / stats[2 * q + 1];
            g = fmaf(dmask[q] * kk * w, fmaf(EX_BETA, v - mask[q], 1.f), g);
        }
        g = wave_sum(g);
        if (lane == 0) {
            const float buf = first ? g : fmaf(mu, mom[c], (1.f - mu) * g);
            mom[c] = buf;
            pmask[c] = fminf(fmaxf(fmaf(-lr, buf, pc), 0.f), 1.f);
        }
    }
}

extern "C" int scouter_extremal_step_f32(float* pmask, float* mom, const float* mask, const float* dmask, const float* stats, int n,
                                         int H, int W, int step, float sigma, float lr, float momentum, int first, void* stream) {
    SC_REQUIRE(pmask && mom && mask && dmask && stats, "extremal_step: null pointer (pmask %p, mom %p, mask %p, dmask %p, stats %p)",
               (void*)pmask, (void*)mom, (const void*)mask, (const void*)dmask, (const void*)stats);
    SC_REQUIRE(n > 0, "extremal_step: n = %d (at least 1)", n);
    ExGeometry g;
    if (int rc = ex_geometry("extremal_step", H, W, step, sigma, g)) return rc;
    SC_REQUIRE(lr >= 0.f && lr <= 3.0e38f && momentum >= 0.f && momentum <= 1.f,
               "extremal_step: lr = %g, momentum = %g (lr finite and not negative, 0 <= momentum <= 1)", (double)lr, (double)momentum);
    SC_REQUIRE(first == 0 || first == 1, "extremal_step: first = %d (0 or 1)", first);
    SC_REQUIRE((((uintptr_t)pmask | (uintptr_t)mom | (uintptr_t)mask | (uintptr_t)dmask | (uintptr_t)stats) & 3) == 0,
               "extremal_step: misaligned pointer (every array must be 4-byte aligned)");
    SC_UNSUPPORTED((double)n * H * W < 1073741824.0, "extremal_step: %d masks of %d x %d pixels are past the 32-bit offsets", n, H, W);
    hipStream_t st = (hipStream_t)stream;
    const long cells_total = (long)n * g.hm * g.wm;
    const double window = (2.0 * g.r + 1.0) * step * (2.0 * g.r + 1.0) * step;
    ScProfScope prof("extremal_step", st, 25.0 * window * (double)cells_total, 4.0 * (4.0 * n * (double)H * W + 4.0 * cells_total));
    hipLaunchKernelGGL(extremal_step_kernel, dim3((unsigned)sc_cdiv(cells_total, EX_WAVES * EX_STEP_CELLS)), dim3(EX_THREADS),
                       (size_t)g.table * sizeof(float), st, pmask, mom, mask, dmask, stats, cells_total, H, W, g.hm, g.wm, step, g.r,
                       sigma, lr, momentum, first);
    return sc_check_launch("extremal_step");
}
