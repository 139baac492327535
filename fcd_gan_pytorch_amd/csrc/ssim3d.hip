// Fused volumetric SSIM level (ssim.py:26-92 on (N,C,T,H,W) inputs, the conv3d branch of gaussian_filter) and the padded
// 2x2x2 average pool between MS-SSIM levels (ssim.py:213-216 with F.avg_pool3d).
//
// Forward: a workgroup owns one (n,c) and one ST3_TY x ST3_TX tile of the OUTPUT plane and walks the depth axis.  Per input
// slice it stages the haloed X,Y patch in LDS and forms the five in-plane window statistics (mu1, mu2, E[x^2], E[y^2], E[xy]:
// H pass, then W pass, as ssim.hip does); each thread then folds the statistics of its two pixels into a shift register of
// per-thread depth accumulators -- slot j holds the partial sum of output slice (t - wst + 1 + j) -- and, once wst slices are
// in, slot 0 is a finished output voxel: ssim/cs are formed in registers and summed in fp64.  X and Y are read once (plus
// halo), nothing of volume size is written: 8 B/voxel instead of the ~30 full-tensor passes of fifteen conv3d calls.
// The reference filters T first; filtering is linear and the products are formed per voxel before any filtering, so T last is
// the same function up to fp32 rounding.
// A dimension shorter than the window is not smoothed (single tap 1, ssim.py:44-50): wst, wsh, wsw are ws or 1, independently.
// Sums: fp64 per workgroup -> part[], reduced per (n,c) in tile order by ssim3d_fin_kernel.  No atomics: run-to-run identical.
// Backward: the same pipeline writes the four adjoint maps (dmu1, dmu2, dB2, de12, each [NC][OT][OH][OW]); the apply kernel
// walks the map slices, runs the transposed (full) window in the plane out of LDS and along depth through the same kind of
// shift register, and applies the X/Y product rule.
#include "common.h"

#define ST3_TY 16
#define ST3_TX 32
#define ST3_WMAX 11
#define ST3_PH (ST3_TY + ST3_WMAX - 1)
#define ST3_PW (ST3_TX + ST3_WMAX - 1)
#define ST3_PIX 2   // output pixels per thread: ST3_TY * ST3_TX / 256

struct Ssim3dGeom {
  int T, H, W, OT, OH, OW, ws, tiles_x, tiles_y;
  int wst, wsh, wsw;   // taps applied along T / H / W: ws, or 1 (identity) when that dimension is shorter than the window
  float C1, C2;
};

// Depth taps of a RING-slot shift register.  Forward (flip = true): slot j collects output slice t - wst + 1 + j from input
// slice t, i.e. tap index wst - 1 - j.  Adjoint (flip = false): slot j collects input slice ot + j from map slice ot, tap j.
// Slots past wst get weight 0; a skipped depth axis (wst = 1 < ws) uses the single tap 1.  (Uniform address arithmetic: these
// live in scalar registers.)
template <int RING>
__device__ __forceinline__ void depth_taps(const float* __restrict__ win, int ws, int wst, bool flip, float (&wt)[RING]) {
#pragma unroll
  for (int j = 0; j < RING; ++j) {
    const bool live = j < wst;
    const int k = live ? (flip ? wst - 1 - j : j) : 0;
    wt[j] = !live ? 0.f : (wst == ws ? win[k] : 1.f);
  }
}

// MODE 0: reduce ssim/cs sums per workgroup -> part[(nc*tiles + tile)*2 + {0,1}]
// MODE 1: write the adjoint maps dmu1, dmu2, dB2, de12 (each [NC][OT][OH][OW]) given per-(n,c) upstream grads
// RING: depth accumulators per statistic and pixel -- 1 when T is not smoothed, ST3_WMAX otherwise
template <int MODE, int RING>
__global__ __launch_bounds__(256) void ssim3d_stats_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                           const float* __restrict__ win, Ssim3dGeom g,
                                                           double* __restrict__ part, const float* __restrict__ g_ssim,
                                                           const float* __restrict__ g_cs, float* __restrict__ maps,
                                                           long long map_stride) {
  __shared__ float sx[ST3_PH * ST3_PW], sy[ST3_PH * ST3_PW];
  __shared__ float vb[5][ST3_TY * ST3_PW];
  __shared__ float wvh[ST3_WMAX], wvw[ST3_WMAX];
  __shared__ double red[16];
  const int tid = threadIdx.x;
  const int nc = blockIdx.z;
  const int oy0 = blockIdx.y * ST3_TY, ox0 = blockIdx.x * ST3_TX;
  const int wsh = g.wsh, wsw = g.wsw, wst = g.wst;
  const int ph = ST3_TY + wsh - 1, pw = ST3_TX + wsw - 1;
  if (tid < g.ws) {
    wvh[tid] = wsh == g.ws ? win[tid] : 1.f;      // (a skipped dimension uses the single tap 1)
    wvw[tid] = wsw == g.ws ? win[tid] : 1.f;
  }
  float wt[RING];
  depth_taps<RING>(win, g.ws, wst, true, wt);
  const long long plane = (long long)g.H * g.W;
  const float* xv = X + (long long)nc * g.T * plane;
  const float* yv = Y + (long long)nc * g.T * plane;
  float acc[ST3_PIX][RING][5];
#pragma unroll
  for (int p = 0; p < ST3_PIX; ++p)
#pragma unroll
    for (int j = 0; j < RING; ++j)
#pragma unroll
      for (int s = 0; s < 5; ++s) acc[p][j][s] = 0.f;
  double s_ssim = 0.0, s_cs = 0.0;
  float gs = 0.f, gc = 0.f;
  if (MODE == 1) {
    const float inv = 1.f / ((float)g.OT * (float)g.OH * (float)g.OW);
    gs = g_ssim[nc] * inv;
    gc = g_cs[nc] * inv;
  }
  const int pr = tid / ST3_TX, pc = tid % ST3_TX;     // pixel p of this thread: row pr + p * (256 / ST3_TX), column pc
  for (int t = 0; t < g.T; ++t) {
    const float* xp = xv + (long long)t * plane;
    const float* yp = yv + (long long)t * plane;
    for (int i = tid; i < ph * pw; i += 256) {
      const int r = i / pw, c = i % pw;
      const int iy = oy0 + r, ix = ox0 + c;
      float a = 0.f, b = 0.f;
      if (iy < g.H && ix < g.W) {
        a = xp[(long long)iy * g.W + ix];
        b = yp[(long long)iy * g.W + ix];
      }
      sx[r * ST3_PW + c] = a;
      sy[r * ST3_PW + c] = b;
    }
    __syncthreads();
    // vertical (H) pass
    for (int i = tid; i < ST3_TY * pw; i += 256) {
      const int r = i / pw, c = i % pw;
      float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
      for (int k = 0; k < wsh; ++k) {
        const float w = wvh[k];
        const float a = sx[(r + k) * ST3_PW + c], b = sy[(r + k) * ST3_PW + c];
        m1 = fmaf(w, a, m1);
        m2 = fmaf(w, b, m2);
        e11 = fmaf(w, a * a, e11);
        e22 = fmaf(w, b * b, e22);
        e12 = fmaf(w, a * b, e12);
      }
      vb[0][r * ST3_PW + c] = m1;
      vb[1][r * ST3_PW + c] = m2;
      vb[2][r * ST3_PW + c] = e11;
      vb[3][r * ST3_PW + c] = e22;
      vb[4][r * ST3_PW + c] = e12;
    }
    __syncthreads();      // (also: every thread is done reading sx/sy before the next slice is staged)
    const int ot = t - wst + 1;
#pragma unroll
    for (int p = 0; p < ST3_PIX; ++p) {
      const int r = pr + p * (256 / ST3_TX), c = pc;
      // horizontal (W) pass, then the depth fold
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        float q = 0.f;
        for (int k = 0; k < wsw; ++k) q = fmaf(wvw[k], vb[s][r * ST3_PW + c + k], q);
#pragma unroll
        for (int j = 0; j < RING; ++j) acc[p][j][s] = RING == 1 ? wt[0] * q : fmaf(wt[j], q, acc[p][j][s]);
      }
      const int oy = oy0 + r, ox = ox0 + c;
      if (ot >= 0 && oy < g.OH && ox < g.OW) {
        const float mu1 = acc[p][0][0], mu2 = acc[p][0][1];
        const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = acc[p][0][2] - mu1s, s2 = acc[p][0][3] - mu2s, s12 = acc[p][0][4] - mu12;
        const float A1 = 2.f * mu12 + g.C1, B1 = mu1s + mu2s + g.C1;
        const float A2 = 2.f * s12 + g.C2, B2 = s1 + s2 + g.C2;
        const float cs = A2 / B2;
        const float l = A1 / B1;
        if (MODE == 0) {
          s_ssim += (double)(l * cs);
          s_cs += (double)cs;
        } else {
          const float G2 = gc + gs * l;   // dL/dcs
          const float Gl = gs * cs;       // dL/dl
          const float dA2 = G2 / B2, dB2 = -G2 * cs / B2;
          const float dA1 = Gl / B1, dB1 = -Gl * l / B1;
          const float de12 = 2.f * dA2;
          const float dmu1 = dA1 * 2.f * mu2 + dB1 * 2.f * mu1 - dB2 * 2.f * mu1 - de12 * mu2;
          const float dmu2 = dA1 * 2.f * mu1 + dB1 * 2.f * mu2 - dB2 * 2.f * mu2 - de12 * mu1;
          const long long o = (((long long)nc * g.OT + ot) * g.OH + oy) * g.OW + ox;
          maps[o] = dmu1;
          maps[map_stride + o] = dmu2;
          maps[2 * map_stride + o] = dB2;
          maps[3 * map_stride + o] = de12;
        }
      }
      // slot 0 is spent: move every partial sum one output slice on
#pragma unroll
      for (int j = 0; j + 1 < RING; ++j)
#pragma unroll
        for (int s = 0; s < 5; ++s) acc[p][j][s] = acc[p][j + 1][s];
#pragma unroll
      for (int s = 0; s < 5; ++s) acc[p][RING - 1][s] = 0.f;
    }
    // (vb is next written after the barrier that follows the staging of slice t + 1)
  }
  if (MODE == 0) {
    s_ssim = block_sum_d(s_ssim, red);
    s_cs = block_sum_d(s_cs, red);
    if (tid == 0) {
      const long long tile = (long long)nc * g.tiles_x * g.tiles_y + (long long)blockIdx.y * g.tiles_x + blockIdx.x;
      part[tile * 2] = s_ssim;
      part[tile * 2 + 1] = s_cs;
    }
  }
}

__global__ void ssim3d_fin_kernel(const double* __restrict__ part, float* __restrict__ out, int NC, int tiles,
                                  double inv_count) {
  const int nc = blockIdx.x * blockDim.x + threadIdx.x;
  if (nc >= NC) return;
  double a = 0.0, b = 0.0;
  for (int t = 0; t < tiles; ++t) {
    a += part[((long long)nc * tiles + t) * 2];
    b += part[((long long)nc * tiles + t) * 2 + 1];
  }
  out[nc] = (float)(a * inv_count);
  out[NC + nc] = (float)(b * inv_count);
}

// transposed window + product rule: one workgroup per (n,c) and ST3_TY x ST3_TX tile of INPUT pixels, walking the depth axis.
// Map slice ot (transposed window in the plane) feeds input slices ot .. ot + wst - 1; slot j of the shift register holds
// the partial sum of input slice ot + j, so after slice `it` of the maps has been folded in, slot 0 is input slice `it`.
template <int RING>
__global__ __launch_bounds__(256) void ssim3d_bwd_apply_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                               const float* __restrict__ win, Ssim3dGeom g,
                                                               const float* __restrict__ maps, long long map_stride,
                                                               float* __restrict__ dX, float* __restrict__ dY) {
  __shared__ float m[4][ST3_PH * ST3_PW];
  __shared__ float vb[4][ST3_TY * ST3_PW];
  __shared__ float wvh[ST3_WMAX], wvw[ST3_WMAX];
  const int tid = threadIdx.x, nc = blockIdx.z;
  const int iy0 = blockIdx.y * ST3_TY, ix0 = blockIdx.x * ST3_TX;
  const int wsh = g.wsh, wsw = g.wsw, halo_h = wsh - 1, halo_w = wsw - 1;
  const int ph = ST3_TY + halo_h, pw = ST3_TX + halo_w;
  if (tid < g.ws) {                               // transposed taps
    wvh[tid] = wsh == g.ws ? win[g.ws - 1 - tid] : 1.f;
    wvw[tid] = wsw == g.ws ? win[g.ws - 1 - tid] : 1.f;
  }
  float wt[RING];
  depth_taps<RING>(win, g.ws, g.wst, false, wt);
  float acc[ST3_PIX][RING][4];
#pragma unroll
  for (int p = 0; p < ST3_PIX; ++p)
#pragma unroll
    for (int j = 0; j < RING; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[p][j][s] = 0.f;
  const long long plane = (long long)g.H * g.W, oplane = (long long)g.OH * g.OW;
  const int pr = tid / ST3_TX, pc = tid % ST3_TX;
  for (int it = 0; it < g.T; ++it) {
    const bool have = it < g.OT;                  // uniform: past the last map slice only the register drains
    if (have) {
      const float* mp = maps + ((long long)nc * g.OT + it) * oplane;
      for (int i = tid; i < ph * pw; i += 256) {
        const int r = i / pw, c = i % pw;
        const int oy = iy0 - halo_h + r, ox = ix0 - halo_w + c;
        const bool ok = oy >= 0 && oy < g.OH && ox >= 0 && ox < g.OW;
        const long long o = ok ? (long long)oy * g.OW + ox : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j][r * ST3_PW + c] = ok ? mp[j * map_stride + o] : 0.f;
      }
      __syncthreads();
      for (int i = tid; i < ST3_TY * pw; i += 256) {
        const int r = i / pw, c = i % pw;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = 0.f;
          for (int k = 0; k < wsh; ++k) a = fmaf(wvh[k], m[j][(r + k) * ST3_PW + c], a);
          vb[j][r * ST3_PW + c] = a;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < ST3_PIX; ++p) {
      const int r = pr + p * (256 / ST3_TX), c = pc;
      if (have) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float u = 0.f;
          for (int k = 0; k < wsw; ++k) u = fmaf(wvw[k], vb[s][r * ST3_PW + c + k], u);
#pragma unroll
          for (int j = 0; j < RING; ++j) acc[p][j][s] = RING == 1 ? wt[0] * u : fmaf(wt[j], u, acc[p][j][s]);
        }
      }
      const int iy = iy0 + r, ix = ix0 + c;
      if (iy < g.H && ix < g.W) {
        const long long o = ((long long)nc * g.T + it) * plane + (long long)iy * g.W + ix;
        const float x = X[o], y = Y[o];
        dX[o] = acc[p][0][0] + 2.f * x * acc[p][0][2] + y * acc[p][0][3];
        dY[o] = acc[p][0][1] + 2.f * y * acc[p][0][2] + x * acc[p][0][3];
      }
#pragma unroll
      for (int j = 0; j + 1 < RING; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[p][j][s] = acc[p][j + 1][s];
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[p][RING - 1][s] = 0.f;
    }
  }
}

static int make_geom3(int T, int H, int W, int win_size, float C1, float C2, Ssim3dGeom* g) {
  if (win_size < 1 || win_size > ST3_WMAX || (win_size & 1) == 0) return -1;
  if (T < 1 || H < 1 || W < 1) return -1;
  g->T = T; g->H = H; g->W = W; g->ws = win_size;
  g->wst = T >= win_size ? win_size : 1;      // gaussian_filter (ssim.py:44-50): no smoothing along a dimension shorter than the window
  g->wsh = H >= win_size ? win_size : 1;
  g->wsw = W >= win_size ? win_size : 1;
  g->OT = T - g->wst + 1; g->OH = H - g->wsh + 1; g->OW = W - g->wsw + 1;
  g->tiles_x = cdiv(g->OW, ST3_TX); g->tiles_y = cdiv(g->OH, ST3_TY);
  g->C1 = C1; g->C2 = C2;
  return 0;
}

// grid limits of the (tiles_x, tiles_y, NC) launch
static bool grid_ok(int NC, int H) { return NC <= 65535 && cdiv(H, ST3_TY) <= 65535; }

extern "C" size_t fcd_ssim3d_ws_bytes(int NC, int T, int H, int W) {
  // max(forward partials: one fp64 {ssim, cs} pair per (n,c) and plane tile; backward: four fp32 adjoint maps, bounded by the
  // input volume)
  if (NC < 1 || T < 1 || H < 1 || W < 1) return 0;
  const size_t fwd = (size_t)NC * cdiv(W, ST3_TX) * cdiv(H, ST3_TY) * 2 * sizeof(double);
  const size_t bwd = (size_t)4 * NC * T * H * W * sizeof(float);
  return std::max(fwd, bwd);
}

extern "C" int fcd_ssim3d_level_fwd(const float* X, const float* Y, const float* win, int win_size, float* out, int NC,
                                    int T, int H, int W, float C1, float C2, void* ws, size_t ws_bytes, void* stream) {
  FCD_CHECK_ARG(X && Y && win && out && NC > 0, "fcd_ssim3d_level_fwd: bad arguments");
  Ssim3dGeom g;
  FCD_CHECK_ARG(make_geom3(T, H, W, win_size, C1, C2, &g) == 0,
                "fcd_ssim3d_level_fwd: window %d unsupported for %dx%dx%d (odd, <= 11)", win_size, T, H, W);
  FCD_CHECK_ARG(grid_ok(NC, H), "fcd_ssim3d_level_fwd: N*C = %d or H = %d beyond the launch grid", NC, H);
  const size_t need = (size_t)NC * g.tiles_x * g.tiles_y * 2 * sizeof(double);
  if (!ws || ws_bytes < need) {
    fcd_set_error("fcd_ssim3d_level_fwd: workspace too small");
    return FCD_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  FcdProfScope prof(FCD_K_LOSS, st, 0.0, 8.0 * NC * (double)T * H * W);
  const dim3 grid(g.tiles_x, g.tiles_y, NC);
  if (g.wst == 1)
    hipLaunchKernelGGL((ssim3d_stats_kernel<0, 1>), grid, dim3(256), 0, st, X, Y, win, g, (double*)ws, (const float*)nullptr,
                       (const float*)nullptr, (float*)nullptr, 0LL);
  else
    hipLaunchKernelGGL((ssim3d_stats_kernel<0, ST3_WMAX>), grid, dim3(256), 0, st, X, Y, win, g, (double*)ws,
                       (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0LL);
  hipLaunchKernelGGL(ssim3d_fin_kernel, dim3(cdiv(NC, 64)), dim3(64), 0, st, (const double*)ws, out, NC,
                     g.tiles_x * g.tiles_y, 1.0 / ((double)g.OT * g.OH * g.OW));
  FCD_LAUNCH_CHECK("ssim3d_level_fwd");
  return FCD_OK;
}

extern "C" int fcd_ssim3d_level_bwd(const float* X, const float* Y, const float* win, int win_size, const float* g_ssim,
                                    const float* g_cs, float* dX, float* dY, int NC, int T, int H, int W, float C1, float C2,
                                    void* ws, size_t ws_bytes, void* stream) {
  FCD_CHECK_ARG(X && Y && win && g_ssim && g_cs && dX && dY && NC > 0, "fcd_ssim3d_level_bwd: bad arguments");
  Ssim3dGeom g;
  FCD_CHECK_ARG(make_geom3(T, H, W, win_size, C1, C2, &g) == 0,
                "fcd_ssim3d_level_bwd: window %d unsupported for %dx%dx%d (odd, <= 11)", win_size, T, H, W);
  FCD_CHECK_ARG(grid_ok(NC, H), "fcd_ssim3d_level_bwd: N*C = %d or H = %d beyond the launch grid", NC, H);
  const long long map_stride = (long long)NC * g.OT * g.OH * g.OW;
  if (!ws || ws_bytes < (size_t)4 * map_stride * sizeof(float)) {
    fcd_set_error("fcd_ssim3d_level_bwd: workspace too small");
    return FCD_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  FcdProfScope prof(FCD_K_LOSS, st, 0.0, 4.0 * NC * (double)T * H * W * 14.0);
  const dim3 grid(g.tiles_x, g.tiles_y, NC), agrid(cdiv(W, ST3_TX), cdiv(H, ST3_TY), NC);
  if (g.wst == 1) {
    hipLaunchKernelGGL((ssim3d_stats_kernel<1, 1>), grid, dim3(256), 0, st, X, Y, win, g, (double*)nullptr, g_ssim, g_cs,
                       (float*)ws, map_stride);
    hipLaunchKernelGGL((ssim3d_bwd_apply_kernel<1>), agrid, dim3(256), 0, st, X, Y, win, g, (const float*)ws, map_stride, dX,
                       dY);
  } else {
    hipLaunchKernelGGL((ssim3d_stats_kernel<1, ST3_WMAX>), grid, dim3(256), 0, st, X, Y, win, g, (double*)nullptr, g_ssim,
                       g_cs, (float*)ws, map_stride);
    hipLaunchKernelGGL((ssim3d_bwd_apply_kernel<ST3_WMAX>), agrid, dim3(256), 0, st, X, Y, win, g, (const float*)ws,
                       map_stride, dX, dY);
  }
  FCD_LAUNCH_CHECK("ssim3d_level_bwd");
  return FCD_OK;
}

// ---- F.avg_pool3d(kernel 2, stride 2, padding = size % 2 per dimension, count_include_pad): divisor always 8 ----
// output size: floor((S + 2p - 2)/2) + 1 ; window of output o covers inputs 2o-p, 2o-p+1
struct Pool3dGeom {
  int T, H, W, OT, P, Q, pt, ph, pw;
};

__global__ void avgpool3d2_pad_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int NC, Pool3dGeom g) {
  const long long total = (long long)NC * g.OT * g.P * g.Q;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % g.Q);
    long long r = i / g.Q;
    const int p = (int)(r % g.P);
    r /= g.P;
    const int o = (int)(r % g.OT);
    const long long pl = r / g.OT;
    const float* s = x + pl * g.T * g.H * g.W;
    double acc = 0.0;      // eight fp32 values sum exactly in fp64: the result is rounded once
    for (int a = 0; a < 2; ++a) {
      const int t = 2 * o - g.pt + a;
      if (t < 0 || t >= g.T) continue;
      for (int b = 0; b < 2; ++b) {
        const int h = 2 * p - g.ph + b;
        if (h < 0 || h >= g.H) continue;
        for (int c = 0; c < 2; ++c) {
          const int w = 2 * q - g.pw + c;
          if (w < 0 || w >= g.W) continue;
          acc += (double)s[((long long)t * g.H + h) * g.W + w];
        }
      }
    }
    y[i] = (float)(acc * 0.125);
  }
}

__global__ void avgpool3d2_pad_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int NC, Pool3dGeom g) {
  const long long total = (long long)NC * g.T * g.H * g.W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int w = (int)(i % g.W);
    long long r = i / g.W;
    const int h = (int)(r % g.H);
    r /= g.H;
    const int t = (int)(r % g.T);
    const long long pl = r / g.T;
    const int o = (t + g.pt) >> 1, p = (h + g.ph) >> 1, q = (w + g.pw) >> 1;
    dx[i] = (o < g.OT && p < g.P && q < g.Q) ? dy[((pl * g.OT + o) * g.P + p) * g.Q + q] * 0.125f : 0.f;
  }
}

static Pool3dGeom pool3d_geom(int T, int H, int W) {
  Pool3dGeom g;
  g.T = T; g.H = H; g.W = W;
  g.pt = T & 1; g.ph = H & 1; g.pw = W & 1;
  g.OT = (T + 2 * g.pt - 2) / 2 + 1; g.P = (H + 2 * g.ph - 2) / 2 + 1; g.Q = (W + 2 * g.pw - 2) / 2 + 1;
  return g;
}

static inline int ew_grid3(long long total) { return (int)std::min<long long>(cdiv64(total, 256), 8192); }

extern "C" int fcd_avgpool3d2_pad_fwd(const float* x, float* y, int NC, int T, int H, int W, void* stream) {
  FCD_CHECK_ARG(x && y && NC > 0, "fcd_avgpool3d2_pad_fwd: bad arguments");
  FCD_CHECK_ARG(T >= 2 && H >= 2 && W >= 2, "fcd_avgpool3d2_pad_fwd: input (T: %d H: %d W: %d) smaller than the 2x2x2 window", T, H, W);
  const Pool3dGeom g = pool3d_geom(T, H, W);
  const long long total = (long long)NC * g.OT * g.P * g.Q;
  FcdProfScope prof(FCD_K_POOL, (hipStream_t)stream, 0.0, 4.0 * NC * 1.125 * T * H * W);
  hipLaunchKernelGGL(avgpool3d2_pad_fwd_kernel, dim3(ew_grid3(total)), dim3(256), 0, (hipStream_t)stream, x, y, NC, g);
  FCD_LAUNCH_CHECK("avgpool3d2_pad_fwd");
  return FCD_OK;
}

extern "C" int fcd_avgpool3d2_pad_bwd(const float* dy, float* dx, int NC, int T, int H, int W, void* stream) {
  FCD_CHECK_ARG(dy && dx && NC > 0, "fcd_avgpool3d2_pad_bwd: bad arguments");
  FCD_CHECK_ARG(T >= 2 && H >= 2 && W >= 2, "fcd_avgpool3d2_pad_bwd: input (T: %d H: %d W: %d) smaller than the 2x2x2 window", T, H, W);
  const Pool3dGeom g = pool3d_geom(T, H, W);
  const long long total = (long long)NC * T * H * W;
  FcdProfScope prof(FCD_K_POOL, (hipStream_t)stream, 0.0, 4.0 * NC * 1.125 * T * H * W);
  hipLaunchKernelGGL(avgpool3d2_pad_bwd_kernel, dim3(ew_grid3(total)), dim3(256), 0, (hipStream_t)stream, dy, dx, NC, g);
  FCD_LAUNCH_CHECK("avgpool3d2_pad_bwd");
  return FCD_OK;
}
