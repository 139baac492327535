// Device-resident scene inference: cut tiles out of a scene pair that lives in HBM, stitch the owned centres of the
// network's density tiles back into scene-sized maps, colour-code them and count the 2x2 confusion matrix -- the data
// movement around the Segmentor in the reference's inference loop (data_utils.py:98-118,205-213,230-236,
// Demo_RSSS.py:345-354,457-491, CommonFunc.py:59-75, metrics.py:67-72).
//
// All three kernels are HBM-bound copies with integer bookkeeping; the only floating-point arithmetic is the fp64
// normalisation of fcd_normalize_tiles.  Geometry comes from a TILE TABLE, int32 (n,12): every row is
// TileGrid.slices(item) flattened -- own x0,y0,w,h | read rx,ry,rw,rh | canvas wx,wy,ww,wh.  The kernels add no tiling
// arithmetic of their own (the reference's border rule lives in ONE place, TileGrid), and they trust the table: the
// caller validates every row on the host before upload (_ops.scene_tile_table).
//
// Work split, all kernels: one wavefront per canvas ROW, lanes along the row -- 64 consecutive dwords = one 256-B
// wave instruction per load / store, whatever the scene width and x0 are (no alignment assumed anywhere, so no vector
// accesses: rows start at arbitrary element offsets in the scene and at r*pw in the canvases).  The grid is 2-D: x = the
// canvas rows in groups of one per wavefront, y = the planes (cut) or tiles (stitch, confusion) behind a grid-stride loop
// capped at the y limit, so any n*planes fits; all offsets into the scene and the canvases are 64-bit.  Wave index, plane
// and table row are wave-uniform (readfirstlane): the decode runs on the scalar unit and the table comes in by scalar loads.
#include <type_traits>

#include "common.h"

enum { T_X0 = 0, T_Y0, T_W, T_H, T_RX, T_RY, T_RW, T_RH, T_WX, T_WY, T_WW, T_WH, T_COLS };

constexpr int kBlock = 256, kWaves = kBlock / FCD_WAVE;                // cut: 4 canvas rows per workgroup
// The counting kernels end in one atomic per counter per WORKGROUP, all on the caller's four counters (one cache line):
// 16 rows per workgroup and at most kCountBlocks workgroups (2 per CU = every wave slot of the chip) keep that to a few
// thousand same-line atomics per launch however large the batch is; further tiles go round the grid-stride loop.
constexpr int kCountBlock = 1024, kCountWaves = kCountBlock / FCD_WAVE, kCountBlocks = 512;
constexpr int kMaxGridY = 65535;       // more planes / tiles than that go round the grid-stride loop

static inline dim3 row_grid(int ph, long long units) { return dim3(cdiv(ph, kWaves), (unsigned)std::min<long long>(units, kMaxGridY)); }
static inline dim3 count_grid(int ph, int n) {
  const int gx = cdiv(ph, kCountWaves);
  return dim3(gx, (unsigned)std::min(n, std::max(1, kCountBlocks / gx)));
}
// canvas row of this wavefront, in a scalar register
template <int WAVES>
__device__ __forceinline__ int wave_row() { return blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// A scene sample as float: exact for all three sample types (uint8 / uint16 fit the 24-bit significand).
__device__ __forceinline__ float load_sample(const void* __restrict__ base, long long idx, int type) {
  if (type == FCD_SAMPLE_U8) return (float)((const uint8_t*)base)[idx];
  if (type == FCD_SAMPLE_U16) return (float)((const uint16_t*)base)[idx];
  return ((const float*)base)[idx];
}

// ---- cut -------------------------------------------------------------------------------------------------------
// One plane of one tile at one canvas row, decoded -- all of it wave-uniform: where the samples come from (``src`` of sample type
// ``type``, canvas column i reads element sbase + i), where the row goes, and what happens on the way.  fcd_scene_cut_kernel and
// the plain fcd_scene_set_cut_kernel decode their planes into this and run cut_row; the _aug instantiation keeps a loop of its own.
struct CutPlane {
  const void* src;
  int type;
  float* dst;
  bool live, norm, ones, region;                   // live: this canvas row holds scene samples (columns wx .. wx + ww)
  double mean, den;
  long long sbase;
  int wx, ww;
};

__device__ __forceinline__ void cut_row(const CutPlane& p, int lane, int pw) {
  for (int i = lane; i < pw; i += FCD_WAVE) {
    float v = 0.f;
    if (p.live && i >= p.wx && i < p.wx + p.ww) {
      if (p.ones) {
        v = 1.f;
      } else {
        v = load_sample(p.src, p.sbase + i, p.type);
        if (p.norm) v = (float)(((double)v - p.mean) / p.den);
        if (p.region && v > 125.f) v = 1.f;                  // data_utils.py:280
      }
    }
    p.dst[i] = v;
  }
}

// planes of one tile: C of x, C of y, [ref], [valid]; one wave per (tile, plane, canvas row).
__global__ __launch_bounds__(kBlock) void fcd_scene_cut_kernel(
    const void* __restrict__ sx, const void* __restrict__ sy, int stype, const void* __restrict__ sref, int rtype, int C,
    long long H, long long W, const int32_t* __restrict__ table, int units, int ph, int pw,
    const double* __restrict__ stats, float* __restrict__ x, float* __restrict__ y, float* __restrict__ ref_tiles,
    float* __restrict__ valid) {
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const unsigned planes = 2 * C + (ref_tiles ? 1 : 0) + (valid ? 1 : 0);
  const int j = wave_row<kWaves>();
  if (j >= ph) return;
  for (unsigned pl = blockIdx.y; pl < (unsigned)units; pl += gridDim.y) {      // units = n * planes <= INT_MAX (checked by the host)
    const long long t = pl / planes;
    const int q = (int)(pl - (unsigned)t * planes);
    const int32_t* __restrict__ row = table + t * T_COLS;
    const int rx = row[T_RX], ry = row[T_RY], wx = row[T_WX], wy = row[T_WY], ww = row[T_WW], wh = row[T_WH];
    // which plane: source, sample type, destination, per-band statistics
    CutPlane p{};
    p.type = stype; p.wx = wx; p.ww = ww; p.den = 1.0;
    p.live = j >= wy && j < wy + wh;
    int c = 0;
    if (q < C) {
      p.src = sx; c = q; p.dst = x + ((t * C + c) * ph + j) * pw; p.norm = stats != nullptr;
    } else if (q < 2 * C) {
      p.src = sy; c = q - C; p.dst = y + ((t * C + c) * ph + j) * pw; p.norm = stats != nullptr;
    } else if (ref_tiles && q == 2 * C) {
      p.src = sref; p.type = rtype; p.dst = ref_tiles + (t * ph + j) * pw;
    } else {
      p.ones = true; p.dst = valid + (t * ph + j) * pw;
    }
    if (p.norm) {        // stats = meanX[C], stdX[C], meanY[C], stdY[C]
      const double* __restrict__ s = stats + (q < C ? 0 : 2 * C);
      p.mean = s[c]; p.den = s[C + c];
    }
    // first sample of the scene row this canvas row reads, shifted so that canvas column i reads element i
    p.sbase = ((long long)c * H + (ry + (j - wy))) * W + (rx - wx);
    cut_row(p, lane, pw);
  }
}

// ---- counting, shared by stitch and tile_confusion -----------------------------------------------------------------
struct SceneCountArgs {
  float thresh, gt0, gt1, pre0, pre1;
};

// cmap > prob_thresh in fp32 (a NaN density is "not changed", as NaN > t is false)
__device__ __forceinline__ float threshold(float p, float thresh) { return p > thresh ? 1.f : 0.f; }

// Evaluator.add_batch_map's four cells, counts[2 * i + j] += (ref == gt_i && pre == pre_j): one ballot + popcount per cell over
// the wavefront (the ballot is 64 bits wide).  Every lane of the wave must call this (inactive pixels pass live = false); the
// running totals are wave-uniform.
__device__ __forceinline__ void count_cells(bool live, float ref, float pre, const SceneCountArgs& a, unsigned long long cnt[4]) {
  cnt[0] += __popcll(__ballot(live && ref == a.gt0 && pre == a.pre0));
  cnt[1] += __popcll(__ballot(live && ref == a.gt0 && pre == a.pre1));
  cnt[2] += __popcll(__ballot(live && ref == a.gt1 && pre == a.pre0));
  cnt[3] += __popcll(__ballot(live && ref == a.gt1 && pre == a.pre1));
}

// wave totals -> workgroup totals in LDS -> ONE ordinary global atomicAdd per counter per workgroup (integer sums: the result does
// not depend on the order the workgroups arrive in)
__device__ __forceinline__ void flush_counts(const unsigned long long cnt[4], unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long part[kCountWaves][4];
  const int lane = threadIdx.x & (FCD_WAVE - 1), w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) part[w][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < kCountWaves; ++k) s += part[k][threadIdx.x];
    if (s) atomicAdd(counts + threadIdx.x, s);
  }
}

// ---- stitch ------------------------------------------------------------------------------------------------------
// one wave per (tile, canvas row j < ph); rows j >= h of a clipped tile have nothing to write.
__global__ __launch_bounds__(kCountBlock) void fcd_scene_stitch_kernel(
    const float* __restrict__ cmap, const int32_t* __restrict__ table, int n, int ph, int pw, int padx, int pady,
    SceneCountArgs a, int write_color, const float* __restrict__ ref, long long W, float* __restrict__ density,
    float* __restrict__ color, unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const int j = wave_row<kCountWaves>();
  unsigned long long cnt[4] = {0, 0, 0, 0};
  for (long long t = blockIdx.y; t < n; t += gridDim.y) {   // no early return: every wave reaches the barrier in flush_counts
    const int32_t* __restrict__ row = table + t * T_COLS;
    const int x0 = row[T_X0], y0 = row[T_Y0], w = row[T_W], h = row[T_H];
    if (j >= h) continue;                                    // wave-uniform (h <= ph - pady: rows past the canvas end here too)
    const float* __restrict__ src = cmap + ((t * ph) + pady + j) * pw + padx;
    const long long obase = (long long)(y0 + j) * W + x0;
    for (int i0 = 0; i0 < w; i0 += FCD_WAVE) {               // wave-uniform trip count: every lane reaches the ballots
      const int i = i0 + lane;
      const bool live = i < w;
      float p = 0.f, g = 0.f;
      if (live) {
        p = src[i];
        if (ref) g = ref[obase + i];
      }
      const float pre = threshold(p, a.thresh);
      float code = 0.f;
      if (write_color && ref) {                              // write_changemap_gdal's assignment order: the later rule wins
        if (pre == a.pre0 && g == a.gt1) code = 1.f;         // miss
        if (pre == a.pre1 && g == a.gt0) code = 2.f;         // false detection
        if (pre == a.pre1 && g == a.gt1) code = 3.f;         // true detection
      } else if (pre == a.pre1) {
        code = 1.f;
      }
      if (live) {
        density[obase + i] = p;
        color[obase + i] = code;
      }
      if (ref && counts) count_cells(live, g, pre, a, cnt);
    }
  }
  if (ref && counts) flush_counts(cnt, counts);
}

// ---- confusion counts over tiles (the training loops' metric) --------------------------------------------------------------
// rects: int32 (n,4) = r0,r1,c0,c1 (TileGrid.eff_range); one wave per (tile, canvas row), rows outside [r0,r1) skipped.
// With ``index`` (fcd_tile_confusion_items) tile t takes row index[t] of a resident table of T rectangles; an index outside the
// table (the host validates the list before upload) counts nothing.
__global__ __launch_bounds__(kCountBlock) void fcd_tile_confusion_kernel(
    const float* __restrict__ cmap, const float* __restrict__ ref_tiles, const int32_t* __restrict__ rects,
    const int32_t* __restrict__ index, int T, int n, int ph, int pw, SceneCountArgs a, unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const int j = wave_row<kCountWaves>();
  unsigned long long cnt[4] = {0, 0, 0, 0};
  for (long long t = blockIdx.y; t < n; t += gridDim.y) {
    const long long g = index ? (long long)index[t] : t;
    if (index && (g < 0 || g >= T)) continue;                // wave-uniform
    const int32_t* __restrict__ rc = rects + g * 4;
    const int r0 = rc[0], r1 = rc[1], c0 = rc[2], c1 = rc[3];
    if (j < r0 || j >= r1) continue;                         // wave-uniform (r1 <= ph)
    const long long base = (t * ph + j) * pw;
    for (int i0 = c0; i0 < c1; i0 += FCD_WAVE) {
      const int i = i0 + lane;
      const bool live = i < c1;
      float p = 0.f, g = 0.f;
      if (live) {
        p = cmap[base + i];
        g = ref_tiles[base + i];
      }
      count_cells(live, g, threshold(p, a.thresh), a, cnt);
    }
  }
  flush_counts(cnt, counts);
}

static bool sample_type_ok(int t) { return t == FCD_SAMPLE_U8 || t == FCD_SAMPLE_U16 || t == FCD_SAMPLE_F32; }
static double sample_bytes(int t) { return t == FCD_SAMPLE_U8 ? 1.0 : t == FCD_SAMPLE_U16 ? 2.0 : 4.0; }

// What the three cut entry points launch over: units = n tiles x planes (C of x, C of y and ``maps`` further canvases), one per
// (blockIdx.y, trip of the grid-stride loop) and counted in 32 bits by the kernels, and the bytes the profiler is told about.
static int cut_work(const char* fn, int sample_type, int C, int maps, int n, int ph, int pw, long long* units, double* bytes) {
  const int planes = 2 * C + maps;
  *units = (long long)n * planes;
  FCD_CHECK_ARG(*units <= INT32_MAX, "%s: %d tiles x %d planes exceed 2^31 - 1", fn, n, planes);
  const long long rows = *units * ph;
  *bytes = (double)rows * pw * 4.0 + 2.0 * n * C * ph * pw * sample_bytes(sample_type);
  return FCD_OK;
}

extern "C" int fcd_scene_cut(const void* scene_x, const void* scene_y, int sample_type, const void* ref, int ref_type, int C,
                             int H, int W, const int32_t* table, int n, int ph, int pw, const double* stats, float* x,
                             float* y, float* ref_tiles, float* valid, void* stream) {
  FCD_CHECK_ARG(scene_x && scene_y && table && x && y && C > 0 && H > 0 && W > 0 && n > 0 && ph > 0 && pw > 0,
                "fcd_scene_cut: bad arguments");
  FCD_CHECK_ARG(sample_type_ok(sample_type), "fcd_scene_cut: sample type %d (0 uint8, 1 uint16, 2 float32)", sample_type);
  FCD_CHECK_ARG((ref != nullptr) == (ref_tiles != nullptr), "fcd_scene_cut: reference map and reference tiles go together");
  FCD_CHECK_ARG(!ref || sample_type_ok(ref_type), "fcd_scene_cut: reference sample type %d", ref_type);
  long long units;
  double bytes;
  const int maps = (ref_tiles ? 1 : 0) + (valid ? 1 : 0);
  if (const int err = cut_work("fcd_scene_cut", sample_type, C, maps, n, ph, pw, &units, &bytes)) return err;
  FcdProfScope prof(FCD_K_MISC, (hipStream_t)stream, 0.0, bytes);
  hipLaunchKernelGGL(fcd_scene_cut_kernel, row_grid(ph, units), dim3(kBlock), 0, (hipStream_t)stream, scene_x, scene_y,
                     sample_type, ref, ref_type, C, (long long)H, (long long)W, table, (int)units, ph, pw, stats, x, y, ref_tiles,
                     valid);
  FCD_LAUNCH_CHECK("fcd_scene_cut");
  return FCD_OK;
}

extern "C" int fcd_scene_stitch(const float* cmap, const int32_t* table, int n, int ph, int pw, int padx, int pady,
                                float thresh, float gt0, float gt1, float pre0, float pre1, int write_color,
                                const float* ref_scene, int H, int W, float* density, float* color,
                                unsigned long long* counts, void* stream) {
  FCD_CHECK_ARG(cmap && table && density && color && n > 0 && ph > 0 && pw > 0 && H > 0 && W > 0 && padx >= 0 && pady >= 0 &&
                    2 * padx < pw && 2 * pady < ph,
                "fcd_scene_stitch: bad arguments");
  const long long rows = (long long)n * ph;
  FcdProfScope prof(FCD_K_MISC, (hipStream_t)stream, 0.0, (double)rows * pw * (ref_scene ? 16.0 : 12.0));
  const SceneCountArgs a{thresh, gt0, gt1, pre0, pre1};
  hipLaunchKernelGGL(fcd_scene_stitch_kernel, count_grid(ph, n), dim3(kCountBlock), 0, (hipStream_t)stream, cmap, table, n, ph, pw,
                     padx, pady, a, write_color, ref_scene, (long long)W, density, color, counts);
  FCD_LAUNCH_CHECK("fcd_scene_stitch");
  return FCD_OK;
}

// both confusion entry points: ``index`` (with T > 0) picks rows of the rectangle table, nullptr takes rectangle t for tile t
static int tile_confusion(const char* fn, const float* cmap, const float* ref_tiles, const int32_t* rects, int T,
                          const int32_t* index, int n, int ph, int pw, const SceneCountArgs& a, unsigned long long* counts,
                          void* stream) {
  FCD_CHECK_ARG(cmap && ref_tiles && rects && counts && n > 0 && ph > 0 && pw > 0, "%s: bad arguments", fn);
  const long long rows = (long long)n * ph;
  FcdProfScope prof(FCD_K_MISC, (hipStream_t)stream, 0.0, (double)rows * pw * 8.0);
  hipLaunchKernelGGL(fcd_tile_confusion_kernel, count_grid(ph, n), dim3(kCountBlock), 0, (hipStream_t)stream, cmap, ref_tiles,
                     rects, index, T, n, ph, pw, a, counts);
  FCD_LAUNCH_CHECK(fn);
  return FCD_OK;
}

extern "C" int fcd_tile_confusion(const float* cmap, const float* ref_tiles, const int32_t* rects, int n, int ph, int pw,
                                  float thresh, float gt0, float gt1, float pre0, float pre1, unsigned long long* counts,
                                  void* stream) {
  return tile_confusion("fcd_tile_confusion", cmap, ref_tiles, rects, 0, nullptr, n, ph, pw, {thresh, gt0, gt1, pre0, pre1}, counts,
                        stream);
}

extern "C" int fcd_tile_confusion_items(const float* cmap, const float* ref_tiles, const int32_t* rect_table, int T,
                                        const int32_t* index, int n, int ph, int pw, float thresh, float gt0, float gt1,
                                        float pre0, float pre1, unsigned long long* counts, void* stream) {
  FCD_CHECK_ARG(index && T > 0, "fcd_tile_confusion_items: bad arguments");
  return tile_confusion("fcd_tile_confusion_items", cmap, ref_tiles, rect_table, T, index, n, ph, pw,
                        {thresh, gt0, gt1, pre0, pre1}, counts, stream);
}

// ==== the training feed: cut from a SET of resident scenes, statistics of a resident scene ===============================
// ---- set cut ---------------------------------------------------------------------------------------------------------
// fcd_scene_cut for tiles drawn from several resident scenes of different (H,W) in one launch.  Three resident inputs: the scene
// descriptors (addresses, sizes, statistics offset), the table of ALL tiles of the set (the 12 columns + the scene index,
// validated per scene on the host before its one upload) and the batch = a list of rows of that table.  planes of one tile:
// C of x, C of y, [ref], [region], [valid]; the decode (index -> row -> scene -> plane) is wave-uniform.  An index outside the
// table or a scene outside the descriptors (neither passes the host's validation) yields a zero tile instead of a wild read.
enum { TS_SCENE = T_COLS, TS_COLS = T_COLS + 1 };

// AUG (fcd_scene_set_cut_aug) adds two things to the x and y planes, nothing to where anything is read or written:
//   * the enhancement MODE (FCD_ENHANCE_*: CommonFunc.NORMALIZE / SCALE / SCALE_NORM) applied to the scenes that have parameters
//     (stats_off >= 0), in fp64 with true divisions in the order the host evaluates them (no reciprocal, no contraction), so that
//     the fp32 result equals NumPy's float64 evaluation followed by .astype(float32) bit for bit;
//   * up to FCD_ERASE_MAX rectangles per tile (x, y, w, h in tile coordinates; w == 0 or h == 0: empty slot), erase[(t*R + r)*4..]:
//     a sample inside any of them is STORED as +0.0f whatever it was (RANDOM_ERASER's assignment).  Lane r holds rectangle r (one
//     16-byte load per lane, issued before the table decode, which it does not depend on); the row test y <= j < y + h is a
//     ballot -- a bit per rectangle in a scalar register, wave-uniform -- and the lanes test x <= i < x + w for the set bits only,
//     with x and w read out of lane r (v_readlane).  Both tests are differences, so no sum of a validated rectangle can overflow.
// AUG = false is the kernel of fcd_scene_set_cut: it compiles without the modes and the rectangle test.
struct SceneAugArgs {
  int mode, R;
  double s0, s1;
  const int32_t* erase;
};

template <bool AUG>
__global__ __launch_bounds__(kBlock) void fcd_scene_set_cut_kernel(
    const fcd_scene_desc* __restrict__ descs, int S, int stype, int C, const int32_t* __restrict__ table, int T,
    const int32_t* __restrict__ index, int units, int ph, int pw, const double* __restrict__ stats, float* __restrict__ x,
    float* __restrict__ y, float* __restrict__ ref_tiles, float* __restrict__ region_tiles, float* __restrict__ valid,
    SceneAugArgs aug) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const unsigned planes = 2 * C + (ref_tiles ? 1 : 0) + (region_tiles ? 1 : 0) + (valid ? 1 : 0);
  const int j = wave_row<kWaves>();
  if (j >= ph) return;
  for (unsigned pl = blockIdx.y; pl < (unsigned)units; pl += gridDim.y) {      // units = n * planes <= INT_MAX (checked by the host)
    const long long t = pl / planes;
    const int q = (int)(pl - (unsigned)t * planes);
    // rectangles of this tile that cross this canvas row: one bit each (x and y planes only; lanes >= R hold an empty slot)
    int4 rect = make_int4(0, 0, 0, 0);
    unsigned long long hit = 0;
    if (AUG && aug.R > 0 && q < 2 * C) {
      if (lane < aug.R) rect = ((const int4*)aug.erase)[t * aug.R + lane];
      hit = __ballot(rect.z > 0 && rect.w > 0 && j >= rect.y && j - rect.y < rect.w);
    }
    const int g = index[t];
    const bool row_ok = g >= 0 && g < T;
    const int32_t* __restrict__ row = table + (long long)(row_ok ? g : 0) * TS_COLS;
    const int s = row[TS_SCENE];
    const bool ok = row_ok && s >= 0 && s < S;
    const fcd_scene_desc* __restrict__ d = descs + (ok ? s : 0);
    const long long H = d->H, W = d->W;
    const int rx = row[T_RX], ry = row[T_RY], wx = row[T_WX], wy = row[T_WY], ww = row[T_WW], wh = row[T_WH];
    CutPlane p{};
    p.type = stype; p.wx = wx; p.ww = ww;
    int c = 0, k = q - 2 * C;
    if (q < C) {
      p.src = (const void*)d->x; c = q; p.dst = x + ((t * C + c) * ph + j) * pw; p.norm = stats != nullptr && d->stats_off >= 0;
    } else if (q < 2 * C) {
      p.src = (const void*)d->y; c = q - C; p.dst = y + ((t * C + c) * ph + j) * pw; p.norm = stats != nullptr && d->stats_off >= 0;
    } else if (ref_tiles && k == 0) {
      p.src = (const void*)d->ref; p.type = d->ref_type; p.dst = ref_tiles + (t * ph + j) * pw;
    } else if (region_tiles && k == (ref_tiles ? 1 : 0)) {
      p.src = (const void*)d->region; p.type = d->region_type; p.region = true; p.dst = region_tiles + (t * ph + j) * pw;
    } else {
      p.ones = true; p.dst = valid + (t * ph + j) * pw;
    }
    if (AUG && aug.mode == FCD_ENHANCE_NONE) p.norm = false;
    double stdv = 1.0;
    if (p.norm) {        // this scene's meanX[C], stdX[C], meanY[C], stdY[C] (AUG, modes 2 and 3: loX, hiX, loY, hiY)
      const double* __restrict__ st = stats + d->stats_off + (q < C ? 0 : 2 * C);
      p.mean = st[c]; stdv = st[C + c];
    }
    // ONE division per sample whatever the mode (all of this is wave-uniform): the divisor is std, or hi - lo for the two scales;
    // SCALE_NORM multiplies the numerator by s1 - s0 first and adds s0 last
    const int mode = AUG ? aug.mode : FCD_ENHANCE_NORMALIZE;
    const bool to_range = AUG && mode == FCD_ENHANCE_SCALE_NORM;
    p.den = mode == FCD_ENHANCE_NORMALIZE ? stdv : stdv - p.mean;
    const double width = AUG ? aug.s1 - aug.s0 : 0.0;
    p.live = ok && j >= wy && j < wy + wh && (p.ones || p.src != nullptr);      // an absent map (address 0) gives zero tiles
    p.sbase = ((long long)c * H + (ry + (j - wy))) * W + (rx - wx);
    if constexpr (!AUG) {
      cut_row(p, lane, pw);
    } else {
      // the row loop of cut_row with the range and the rectangles, kept apart: merged into cut_row this instantiation measured
      // outside the spread of the separate loop (profiles/scene_refactor.md)
      for (int i = lane; i < pw; i += FCD_WAVE) {
        float v = 0.f;
        if (p.live && i >= wx && i < wx + ww) {
          if (p.ones) {
            v = 1.f;
          } else {
            v = load_sample(p.src, p.sbase + i, p.type);
            if (p.norm) {
              double e = (double)v - p.mean;
              if (to_range) e = width * e;
              e = e / p.den;
              if (to_range) e = e + aug.s0;
              v = (float)e;
            }
            if (p.region && v > 125.f) v = 1.f;                // data_utils.py:280
          }
        }
        bool gone = false;
        for (unsigned long long m = hit; m; m &= m - 1) {      // wave-uniform trip count
          const int r = __builtin_ctzll(m);
          const int ex = __builtin_amdgcn_readlane(rect.x, r), ew = __builtin_amdgcn_readlane(rect.z, r);
          gone = gone || (i >= ex && i - ex < ew);
        }
        if (gone) v = 0.f;                                     // an assignment: NaN and inf become +0 too
        p.dst[i] = v;
      }
    }
  }
}

// both set-cut entry points; the plain one passes empty SceneAugArgs to the AUG = false instantiation
template <bool AUG>
static int set_cut(const char* fn, const fcd_scene_desc* descs, int S, int sample_type, int C, const int32_t* table, int T,
                   const int32_t* index, int n, int ph, int pw, const double* stats, const SceneAugArgs& aug, float* x, float* y,
                   float* ref_tiles, float* region_tiles, float* valid, void* stream) {
  FCD_CHECK_ARG(descs && table && index && x && y && S > 0 && C > 0 && T > 0 && n > 0 && ph > 0 && pw > 0, "%s: bad arguments", fn);
  FCD_CHECK_ARG(sample_type_ok(sample_type), "%s: sample type %d (0 uint8, 1 uint16, 2 float32)", fn, sample_type);
  if (AUG) {
    FCD_CHECK_ARG(aug.mode >= FCD_ENHANCE_NONE && aug.mode <= FCD_ENHANCE_SCALE_NORM,
                  "%s: enhancement mode %d (0 none, 1 normalize, 2 scale, 3 scale_norm)", fn, aug.mode);
    FCD_CHECK_ARG(aug.R >= 0 && aug.R <= FCD_ERASE_MAX, "%s: %d rectangles per tile, at most %d", fn, aug.R, FCD_ERASE_MAX);
    FCD_CHECK_ARG((aug.erase != nullptr) == (aug.R > 0), "%s: the rectangle list goes with R > 0 (R = %d)", fn, aug.R);
    FCD_CHECK_ARG(((uintptr_t)aug.erase & 15) == 0, "%s: the rectangle list must be 16-byte aligned", fn);
  }
  long long units;
  double bytes;
  const int maps = (ref_tiles ? 1 : 0) + (region_tiles ? 1 : 0) + (valid ? 1 : 0);
  if (const int err = cut_work(fn, sample_type, C, maps, n, ph, pw, &units, &bytes)) return err;
  FcdProfScope prof(FCD_K_MISC, (hipStream_t)stream, 0.0, bytes);
  hipLaunchKernelGGL(fcd_scene_set_cut_kernel<AUG>, row_grid(ph, units), dim3(kBlock), 0, (hipStream_t)stream, descs, S,
                     sample_type, C, table, T, index, (int)units, ph, pw, stats, x, y, ref_tiles, region_tiles, valid, aug);
  FCD_LAUNCH_CHECK(fn);
  return FCD_OK;
}

extern "C" int fcd_scene_set_cut(const fcd_scene_desc* descs, int S, int sample_type, int C, const int32_t* table, int T,
                                 const int32_t* index, int n, int ph, int pw, const double* stats, float* x, float* y,
                                 float* ref_tiles, float* region_tiles, float* valid, void* stream) {
  return set_cut<false>("fcd_scene_set_cut", descs, S, sample_type, C, table, T, index, n, ph, pw, stats, SceneAugArgs{}, x, y,
                        ref_tiles, region_tiles, valid, stream);
}

extern "C" int fcd_scene_set_cut_aug(const fcd_scene_desc* descs, int S, int sample_type, int C, const int32_t* table, int T,
                                     const int32_t* index, int n, int ph, int pw, const double* stats, int mode, double s0,
                                     double s1, const int32_t* erase, int R, float* x, float* y, float* ref_tiles,
                                     float* region_tiles, float* valid, void* stream) {
  return set_cut<true>("fcd_scene_set_cut_aug", descs, S, sample_type, C, table, T, index, n, ph, pw, stats,
                       SceneAugArgs{mode, R, s0, s1, erase}, x, y, ref_tiles, region_tiles, valid, stream);
}

// ---- set stitch ------------------------------------------------------------------------------------------------------
// fcd_scene_stitch for a batch whose tiles come from S resident scenes: the inference side of the set.  The maps of all scenes
// lie end to end in ONE density and ONE colour buffer, scene s at [map_off[s], map_off[s + 1]); the counters are one row of four
// per scene.  One wave per (tile, canvas row); the decode index -> row -> scene -> map offset is wave-uniform, and more than
// that: t depends on blockIdx.y alone, so all 16 waves of a workgroup walk the same tiles and "the scene of this tile differs
// from the last one's" is WORKGROUP-uniform.  The running totals are flushed through flush_counts at every such change (and at
// the end) into the row of the scene they belong to; every wave reaches those barriers the same number of times because the row
// test j >= h comes AFTER the flush.  A tile whose index, scene, map span or owned rectangle does not fit (none passes the
// host's validation) is skipped as a whole: no store, no count -- and, being a function of t too, no divergent barrier.
__global__ __launch_bounds__(kCountBlock) void fcd_scene_set_stitch_kernel(
    const float* __restrict__ cmap, const fcd_scene_desc* __restrict__ descs, int S, const int32_t* __restrict__ table, int T,
    const int32_t* __restrict__ index, int n, int ph, int pw, int padx, int pady, SceneCountArgs a, int write_color,
    const long long* __restrict__ map_off, long long total, float* __restrict__ density, float* __restrict__ color,
    unsigned long long* __restrict__ scene_counts) {
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const int j = wave_row<kCountWaves>();
  unsigned long long cnt[4] = {0, 0, 0, 0};
  int cur = -1;                                              // the scene cnt belongs to; workgroup-uniform
  for (long long t = blockIdx.y; t < n; t += gridDim.y) {
    const int g = index[t];
    const bool row_ok = g >= 0 && g < T;
    const int32_t* __restrict__ row = table + (long long)(row_ok ? g : 0) * TS_COLS;
    const int s = row[TS_SCENE];
    bool ok = row_ok && s >= 0 && s < S;
    const fcd_scene_desc* __restrict__ d = descs + (ok ? s : 0);
    const long long H = d->H, W = d->W;
    const long long off = map_off[ok ? s : 0], end = map_off[(ok ? s : 0) + 1];
    const int x0 = row[T_X0], y0 = row[T_Y0], w = row[T_W], h = row[T_H];
    ok = ok && off >= 0 && end <= total && H > 0 && W > 0 && end - off == H * W;
    ok = ok && x0 >= 0 && y0 >= 0 && w >= 0 && h >= 0 && (long long)x0 + w <= W && (long long)y0 + h <= H && padx + w <= pw &&
         pady + h <= ph;
    if (!ok) continue;                                       // workgroup-uniform: a function of t alone
    const bool has_ref = d->ref != 0;
    const bool counting = has_ref && scene_counts != nullptr;
    if (counting && s != cur) {                              // workgroup-uniform, in front of the row test: all waves flush
      if (cur >= 0) {
        flush_counts(cnt, scene_counts + (long long)cur * 4);
        __syncthreads();                                     // the LDS partials are free for the next flush
        cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
      }
      cur = s;
    }
    if (j >= h) continue;                                    // wave-uniform; no barrier between here and the next tile
    const float* __restrict__ src = cmap + ((t * ph) + pady + j) * pw + padx;
    const long long rbase = (long long)(y0 + j) * W + x0;    // inside the scene's reference map
    const long long obase = off + rbase;                     // inside the flat maps
    const void* __restrict__ ref = (const void*)d->ref;
    const int rtype = d->ref_type;
    for (int i0 = 0; i0 < w; i0 += FCD_WAVE) {               // wave-uniform trip count: every lane reaches the ballots
      const int i = i0 + lane;
      const bool live = i < w;
      float p = 0.f, gt = 0.f;
      if (live) {
        p = src[i];
        if (has_ref) gt = load_sample(ref, rbase + i, rtype);
      }
      const float pre = threshold(p, a.thresh);
      float code = 0.f;
      if (write_color && has_ref) {                          // write_changemap_gdal's assignment order: the later rule wins
        if (pre == a.pre0 && gt == a.gt1) code = 1.f;        // miss
        if (pre == a.pre1 && gt == a.gt0) code = 2.f;        // false detection
        if (pre == a.pre1 && gt == a.gt1) code = 3.f;        // true detection
      } else if (pre == a.pre1) {
        code = 1.f;
      }
      if (live) {
        density[obase + i] = p;
        color[obase + i] = code;
      }
      if (counting) count_cells(live, gt, pre, a, cnt);
    }
  }
  if (scene_counts && cur >= 0) flush_counts(cnt, scene_counts + (long long)cur * 4);     // workgroup-uniform
}

extern "C" int fcd_scene_set_stitch(const float* cmap, const fcd_scene_desc* descs, int S, const int32_t* table, int T,
                                    const int32_t* index, int n, int ph, int pw, int padx, int pady, float thresh, float gt0,
                                    float gt1, float pre0, float pre1, int write_color, const int64_t* map_off, int64_t total,
                                    float* density, float* color, unsigned long long* scene_counts, void* stream) {
  FCD_CHECK_ARG(cmap && descs && table && index && map_off && density && color && S > 0 && T > 0 && n > 0 && ph > 0 && pw > 0 &&
                    total > 0 && padx >= 0 && pady >= 0 && 2 * padx < pw && 2 * pady < ph,
                "fcd_scene_set_stitch: bad arguments");
  const long long rows = (long long)n * ph;
  FcdProfScope prof(FCD_K_MISC, (hipStream_t)stream, 0.0, (double)rows * pw * 16.0);
  const SceneCountArgs a{thresh, gt0, gt1, pre0, pre1};
  hipLaunchKernelGGL(fcd_scene_set_stitch_kernel, count_grid(ph, n), dim3(kCountBlock), 0, (hipStream_t)stream, cmap, descs, S,
                     table, T, index, n, ph, pw, padx, pady, a, write_color, (const long long*)map_off, (long long)total, density,
                     color, scene_counts);
  FCD_LAUNCH_CHECK("fcd_scene_set_stitch");
  return FCD_OK;
}

// ---- the masked scan of the statistics and the extrema -------------------------------------------------------------------
// Both go over the read rectangles of a tile table under one mask: a pixel counts when the fp32 band sum of scene x is non-zero
// (NaN != 0: counts), for both scenes, once per tile that reads it.  One wave per (tile, row of the read rectangle): the mask of
// up to 64 x 64 columns is kept as one bit per chunk in a 64-bit register per lane, then every band is read once more under it.
constexpr int kStatBands = 32;                                         // 16 waves x (1 + 4 * 32) slots x 8 B = 16.1 KB of LDS
constexpr int kStatSegment = FCD_WAVE * 64;                            // columns one mask register per lane covers

// v combined over the wavefront by ``op(mine, other lane's)`` (xor butterfly: every lane ends with the result)
template <typename T, typename OP>
__device__ __forceinline__ T wave_reduce(T v, OP op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
struct OpSum { __device__ unsigned long long operator()(unsigned long long v, unsigned long long u) const { return v + u; } };
struct OpMin { __device__ float operator()(float v, float u) const { return u < v ? u : v; } };     // a NaN u never replaces v
struct OpMax { __device__ float operator()(float v, float u) const { return u > v ? u : v; } };
__device__ __forceinline__ unsigned long long wave_total(unsigned long long v) { return wave_reduce(v, OpSum()); }
__device__ __forceinline__ double wave_total(double v) { return wave_sum_d(v); }

// The walk, written once.  Per 4096-column segment of a row: ``count(n)`` on lane 0 with the wave's number of valid pixels, then
// for every band c a default-constructed LANE that takes ``sample(l, c, vx, vy)`` for each valid column of this lane, in column
// order, and ends in ``band(l, c)``, called by all 64 lanes (it reduces over the wave).  The callers say what they accumulate and
// where they keep it; nothing here returns early, so every wave reaches the caller's barrier.
template <typename LANE, typename COUNT, typename SAMPLE, typename BAND>
__device__ __forceinline__ void masked_scan(const void* __restrict__ sx, const void* __restrict__ sy, int stype, int C, long long H,
                                            long long W, const int32_t* __restrict__ table, int n, int lane, int j, COUNT count,
                                            SAMPLE sample, BAND band) {
  for (long long t = blockIdx.y; t < n; t += gridDim.y) {
    const int32_t* __restrict__ row = table + t * T_COLS;
    const int rx = row[T_RX], ry = row[T_RY], rw = row[T_RW], rh = row[T_RH];
    if (j >= rh) continue;                                    // wave-uniform
    const long long rbase = (long long)(ry + j) * W + rx;    // first sample of this row in band 0
    for (int seg = 0; seg < rw; seg += kStatSegment) {
      const int chunks = std::min(64, (rw - seg + FCD_WAVE - 1) / FCD_WAVE);
      unsigned long long bits = 0;                           // bit k: column seg + 64 k + lane is valid
      for (int k = 0; k < chunks; ++k) {
        const int i = seg + k * FCD_WAVE + lane;
        if (i < rw) {
          float s = 0.f;
          for (int c = 0; c < C; ++c) s += load_sample(sx, (long long)c * H * W + rbase + i, stype);
          if (s != 0.f) bits |= 1ull << k;
        }
      }
      const unsigned long long cnt = wave_total((unsigned long long)__popcll(bits));
      if (lane == 0) count(cnt);
      for (int c = 0; c < C; ++c) {
        LANE l;
        const long long cbase = (long long)c * H * W + rbase;
        for (int k = 0; k < chunks; ++k) {
          if (!((bits >> k) & 1)) continue;
          const int i = seg + k * FCD_WAVE + lane;
          sample(l, c, load_sample(sx, cbase + i, stype), load_sample(sy, cbase + i, stype));
        }
        band(l, c);
      }
    }
  }
}

// ---- statistics ------------------------------------------------------------------------------------------------------
// Masked per-band moments (CommonFunc.Dataset_mean / Dataset_std, CommonFunc.py:436-500).  Lane totals -> wave total (shuffles)
// -> the wave's OWN slots in LDS (plain adds, no atomics, in the fixed order of the wave's tiles) -> workgroup total, summed over
// the waves in index order.
//   MODE 0, uint8 / uint16: n, sum x[C], sum x^2[C], sum y[C], sum y^2[C] as exact unsigned 64-bit integers at every level; the
//           workgroup totals go to the caller's totals by integer atomics (order-independent, so run-to-run identical).
//   MODE 1, float32 pass 1: n, sum x[C], sum y[C] in fp64, one partial row per workgroup in the workspace.
//   MODE 2, float32 pass 2: sum (x - mean)^2[C], sum (y - mean)^2[C] about the fp64 means of pass 1, partials likewise.
// The partial rows are folded in index order by fcd_scene_stats_fold_kernel: no floating-point atomics anywhere, and the grid
// depends on (n, ph) only, so two runs agree bit for bit.
template <int MODE>
__global__ __launch_bounds__(kCountBlock) void fcd_scene_stats_kernel(
    const void* __restrict__ sx, const void* __restrict__ sy, int stype, int C, long long H, long long W,
    const int32_t* __restrict__ table, int n, const double* __restrict__ mean, void* __restrict__ out) {
  typedef typename std::conditional<MODE == 0, unsigned long long, double>::type acc_t;
  __shared__ acc_t part[kCountWaves][1 + 4 * kStatBands];
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j = wave_row<kCountWaves>();
  const int slots = MODE == 0 ? 1 + 4 * C : MODE == 1 ? 1 + 2 * C : 2 * C;
  for (int k = lane; k < slots; k += FCD_WAVE) part[w][k] = 0;
  __syncthreads();
  if constexpr (MODE == 0) {
    // the integer moments keep a walk of their own, the one masked_scan has: merged into it this instantiation measured outside
    // the spread of the separate loop (profiles/scene_refactor.md)
    for (long long t = blockIdx.y; t < n; t += gridDim.y) {  // no early return: every wave reaches the barrier below
      const int32_t* __restrict__ row = table + t * T_COLS;
      const int rx = row[T_RX], ry = row[T_RY], rw = row[T_RW], rh = row[T_RH];
      if (j >= rh) continue;                                  // wave-uniform
      const long long rbase = (long long)(ry + j) * W + rx;
      for (int seg = 0; seg < rw; seg += kStatSegment) {
        const int chunks = std::min(64, (rw - seg + FCD_WAVE - 1) / FCD_WAVE);
        unsigned long long bits = 0;
        for (int k = 0; k < chunks; ++k) {
          const int i = seg + k * FCD_WAVE + lane;
          if (i < rw) {
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += load_sample(sx, (long long)c * H * W + rbase + i, stype);
            if (s != 0.f) bits |= 1ull << k;
          }
        }
        const acc_t cnt = wave_total((acc_t)__popcll(bits));
        if (lane == 0) part[w][0] += cnt;
        for (int c = 0; c < C; ++c) {
          acc_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
          const long long cbase = (long long)c * H * W + rbase;
          for (int k = 0; k < chunks; ++k) {
            if (!((bits >> k) & 1)) continue;
            const int i = seg + k * FCD_WAVE + lane;
            const float vx = load_sample(sx, cbase + i, stype), vy = load_sample(sy, cbase + i, stype);
            const acc_t ux = (acc_t)(unsigned)vx, uy = (acc_t)(unsigned)vy;   // uint8 / uint16 samples: exact in float, exact back
            a0 += ux; a1 += ux * ux; b0 += uy; b1 += uy * uy;
          }
          a0 = wave_total(a0); b0 = wave_total(b0); a1 = wave_total(a1); b1 = wave_total(b1);
          if (lane == 0) {
            part[w][1 + c] += a0; part[w][1 + C + c] += a1; part[w][1 + 2 * C + c] += b0; part[w][1 + 3 * C + c] += b1;
          }
        }
      }
    }
  } else {
    struct Lane {
      double a0 = 0, b0 = 0;                                 // sums over x and over y
    };
    masked_scan<Lane>(
        sx, sy, stype, C, H, W, table, n, lane, j,
        [&](unsigned long long cnt) { if (MODE == 1) part[w][0] += (double)cnt; },    // a count is exact in fp64 too
        [&](Lane& l, int c, float vx, float vy) {
          if (MODE == 1) {
            l.a0 += (double)vx; l.b0 += (double)vy;
          } else {
            const double dx = (double)vx - mean[c], dy = (double)vy - mean[C + c];
            l.a0 += dx * dx; l.b0 += dy * dy;
          }
        },
        [&](Lane& l, int c) {
          const double a0 = wave_total(l.a0), b0 = wave_total(l.b0);
          const int at = MODE == 1 ? 1 : 0;
          if (lane == 0) { part[w][at + c] += a0; part[w][at + C + c] += b0; }
        });
  }
  __syncthreads();
  if ((int)threadIdx.x < slots) {
    acc_t s = 0;
    for (int k = 0; k < kCountWaves; ++k) s += part[k][threadIdx.x];
    if (MODE == 0) {
      if (s) atomicAdd((unsigned long long*)out + threadIdx.x, (unsigned long long)s);
    } else {
      ((double*)out)[((long long)blockIdx.y * gridDim.x + blockIdx.x) * slots + threadIdx.x] = (double)s;
    }
  }
}

// out[k] = sum over the workgroups' partial rows, in index order; with ``means`` slot 0 is the count n and every other slot is
// divided by it.
__global__ __launch_bounds__(kBlock) void fcd_scene_stats_fold_kernel(const double* __restrict__ partials, int blocks, int slots,
                                                                     int means, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= slots) return;
  double s = 0.0, cnt = 0.0;
  for (int b = 0; b < blocks; ++b) {
    s += partials[(long long)b * slots + k];
    if (means) cnt += partials[(long long)b * slots];
  }
  out[k] = means && k > 0 ? s / cnt : s;
}

static inline int stats_blocks(int n, int ph) {
  const dim3 g = count_grid(ph, n);
  return (int)(g.x * g.y);
}

extern "C" size_t fcd_scene_stats_ws_bytes(int sample_type, int C, int n, int ph) {
  if (sample_type != FCD_SAMPLE_F32 || C <= 0 || C > kStatBands || n <= 0 || ph <= 0) return 0;
  return (size_t)stats_blocks(n, ph) * (1 + 2 * C) * sizeof(double);
}

extern "C" int fcd_scene_stats(const void* scene_x, const void* scene_y, int sample_type, int C, int H, int W,
                               const int32_t* table, int n, int ph, int pw, void* out, void* ws, size_t ws_bytes, void* stream) {
  FCD_CHECK_ARG(scene_x && scene_y && table && out && C > 0 && H > 0 && W > 0 && n > 0 && ph > 0 && pw > 0,
                "fcd_scene_stats: bad arguments");
  FCD_CHECK_ARG(sample_type_ok(sample_type), "fcd_scene_stats: sample type %d (0 uint8, 1 uint16, 2 float32)", sample_type);
  FCD_CHECK_ARG(C <= kStatBands, "fcd_scene_stats: %d bands, at most %d", C, kStatBands);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = count_grid(ph, n);
  const double bytes = (double)n * ph * pw * (3.0 * C) * sample_bytes(sample_type);
  if (sample_type != FCD_SAMPLE_F32) {
    const unsigned long long vmax = sample_type == FCD_SAMPLE_U8 ? 255ull : 65535ull;
    const unsigned long long pixels = (unsigned long long)n * (unsigned long long)ph * (unsigned long long)pw;
    FCD_CHECK_ARG(pixels < UINT64_MAX / (vmax * vmax), "fcd_scene_stats: %d tiles of %dx%d: the sum of squares may exceed 2^64", n,
                  pw, ph);
    FcdProfScope prof(FCD_K_MISC, st, 0.0, bytes);
    if (hipMemsetAsync(out, 0, (size_t)(1 + 4 * C) * sizeof(unsigned long long), st) != hipSuccess) {
      fcd_set_error("fcd_scene_stats: clearing the totals failed");
      return FCD_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(fcd_scene_stats_kernel<0>, grid, dim3(kCountBlock), 0, st, scene_x, scene_y, sample_type, C, (long long)H,
                       (long long)W, table, n, (const double*)nullptr, out);
    FCD_LAUNCH_CHECK("fcd_scene_stats");
    return FCD_OK;
  }
  const size_t need = fcd_scene_stats_ws_bytes(sample_type, C, n, ph);
  FCD_CHECK_ARG(ws && ws_bytes >= need, "fcd_scene_stats: workspace of %zu bytes, %zu needed", ws_bytes, need);
  FcdProfScope prof(FCD_K_MISC, st, 0.0, 2.0 * bytes);
  const int blocks = (int)(grid.x * grid.y);
  double* o = (double*)out;                                  // n | meanX[C] meanY[C] | ssX[C] ssY[C]
  hipLaunchKernelGGL(fcd_scene_stats_kernel<1>, grid, dim3(kCountBlock), 0, st, scene_x, scene_y, sample_type, C, (long long)H,
                     (long long)W, table, n, (const double*)nullptr, ws);
  hipLaunchKernelGGL(fcd_scene_stats_fold_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ws, blocks, 1 + 2 * C, 1, o);
  hipLaunchKernelGGL(fcd_scene_stats_kernel<2>, grid, dim3(kCountBlock), 0, st, scene_x, scene_y, sample_type, C, (long long)H,
                     (long long)W, table, n, (const double*)(o + 1), ws);
  hipLaunchKernelGGL(fcd_scene_stats_fold_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ws, blocks, 2 * C, 0, o + 1 + 2 * C);
  FCD_LAUNCH_CHECK("fcd_scene_stats");
  return FCD_OK;
}

// ---- extrema ---------------------------------------------------------------------------------------------------------
// Masked per-band minimum and maximum of both scenes over the read rectangles of a tile table (CommonFunc.Dataset_maxmin,
// CommonFunc.py:294-370): the masked scan with min / max in place of sums -- wave reduction (shuffles), the wave's OWN slots in
// LDS, one partial row per workgroup.  Every sample type goes through float: uint8 and uint16 are exact there, so ONE kernel
// serves all three and there is no atomic of any kind; the partial rows (4*C floats and a 64-bit count per workgroup) are folded
// by fcd_scene_minmax_fold_kernel.  A sample replaces the running extremum only when it compares below / above it, so a NaN
// sample is skipped and +-inf take part; the running values start at +inf / -inf, which is what a band without a single
// comparable sample returns.
__global__ __launch_bounds__(kCountBlock) void fcd_scene_minmax_kernel(
    const void* __restrict__ sx, const void* __restrict__ sy, int stype, int C, long long H, long long W,
    const int32_t* __restrict__ table, int n, float* __restrict__ part_out, unsigned long long* __restrict__ cnt_out) {
  __shared__ float part[kCountWaves][4 * kStatBands];        // minX[C] maxX[C] minY[C] maxY[C] per wave: 8 KB
  __shared__ unsigned long long pcnt[kCountWaves];
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j = wave_row<kCountWaves>();
  const int slots = 4 * C;
  for (int k = lane; k < slots; k += FCD_WAVE) part[w][k] = ((k / C) & 1) ? -INFINITY : INFINITY;
  if (lane == 0) pcnt[w] = 0;
  __syncthreads();
  const OpMin lo;
  const OpMax hi;
  struct Lane {
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
  };
  masked_scan<Lane>(
      sx, sy, stype, C, H, W, table, n, lane, j, [&](unsigned long long cnt) { pcnt[w] += cnt; },
      [&](Lane& l, int, float vx, float vy) {
        l.x0 = lo(l.x0, vx); l.x1 = hi(l.x1, vx); l.y0 = lo(l.y0, vy); l.y1 = hi(l.y1, vy);
      },
      [&](Lane& l, int c) {
        const float x0 = wave_reduce(l.x0, lo), x1 = wave_reduce(l.x1, hi), y0 = wave_reduce(l.y0, lo), y1 = wave_reduce(l.y1, hi);
        if (lane == 0) {
          part[w][c] = lo(part[w][c], x0); part[w][C + c] = hi(part[w][C + c], x1);
          part[w][2 * C + c] = lo(part[w][2 * C + c], y0); part[w][3 * C + c] = hi(part[w][3 * C + c], y1);
        }
      });
  __syncthreads();
  const long long block = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  if ((int)threadIdx.x < slots) {
    const bool is_max = ((int)threadIdx.x / C) & 1;
    float v = part[0][threadIdx.x];
    for (int k = 1; k < kCountWaves; ++k) {
      const float u = part[k][threadIdx.x];
      v = is_max ? hi(v, u) : lo(v, u);
    }
    part_out[block * slots + threadIdx.x] = v;
  } else if ((int)threadIdx.x == slots) {                    // slots <= 128 < the block size
    unsigned long long s = 0;
    for (int k = 0; k < kCountWaves; ++k) s += pcnt[k];
    cnt_out[block] = s;
  }
}

// out[k] = min / max over the workgroups' partial rows (rows 0 and 2 of the (4,C) result are minima), count = sum of their counts.
// One wave per output: the lanes stride over the partial rows (a few loads each, all in flight together) and reduce by shuffles;
// workgroup 4*C folds the counts.
__global__ __launch_bounds__(FCD_WAVE) void fcd_scene_minmax_fold_kernel(const float* __restrict__ partials,
                                                                        const unsigned long long* __restrict__ counts, int blocks,
                                                                        int C, float* __restrict__ out,
                                                                        unsigned long long* __restrict__ count) {
  const int k = blockIdx.x, slots = 4 * C, lane = threadIdx.x;
  if (k < slots) {
    const bool is_max = (k / C) & 1;                         // uniform over the workgroup
    float v = is_max ? -INFINITY : INFINITY;
    for (int b = lane; b < blocks; b += FCD_WAVE) {
      const float u = partials[(long long)b * slots + k];
      v = is_max ? OpMax()(v, u) : OpMin()(v, u);
    }
    v = is_max ? wave_reduce(v, OpMax()) : wave_reduce(v, OpMin());
    if (lane == 0) out[k] = v;
  } else {
    unsigned long long s = 0;
    for (int b = lane; b < blocks; b += FCD_WAVE) s += counts[b];
    s = wave_total(s);
    if (lane == 0) *count = s;
  }
}

// workspace: blocks x 4*C floats (16*C bytes per row: the counts behind them stay 8-byte aligned), then blocks x one 64-bit count
extern "C" size_t fcd_scene_minmax_ws_bytes(int C, int n, int ph) {
  if (C <= 0 || C > kStatBands || n <= 0 || ph <= 0) return 0;
  return (size_t)stats_blocks(n, ph) * ((size_t)4 * C * sizeof(float) + sizeof(unsigned long long));
}

extern "C" int fcd_scene_minmax(const void* scene_x, const void* scene_y, int sample_type, int C, int H, int W,
                                const int32_t* table, int n, int ph, int pw, float* out, unsigned long long* count, void* ws,
                                size_t ws_bytes, void* stream) {
  FCD_CHECK_ARG(scene_x && scene_y && table && out && count && C > 0 && H > 0 && W > 0 && n > 0 && ph > 0 && pw > 0,
                "fcd_scene_minmax: bad arguments");
  FCD_CHECK_ARG(sample_type_ok(sample_type), "fcd_scene_minmax: sample type %d (0 uint8, 1 uint16, 2 float32)", sample_type);
  FCD_CHECK_ARG(C <= kStatBands, "fcd_scene_minmax: %d bands, at most %d", C, kStatBands);
  const size_t need = fcd_scene_minmax_ws_bytes(C, n, ph);
  FCD_CHECK_ARG(ws && ws_bytes >= need, "fcd_scene_minmax: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = count_grid(ph, n);
  const int blocks = (int)(grid.x * grid.y);
  float* parts = (float*)ws;
  unsigned long long* counts = (unsigned long long*)((char*)ws + (size_t)blocks * 4 * C * sizeof(float));
  const double bytes = (double)n * ph * pw * (3.0 * C) * sample_bytes(sample_type);
  FcdProfScope prof(FCD_K_MISC, st, 0.0, bytes);
  hipLaunchKernelGGL(fcd_scene_minmax_kernel, grid, dim3(kCountBlock), 0, st, scene_x, scene_y, sample_type, C, (long long)H,
                     (long long)W, table, n, parts, counts);
  hipLaunchKernelGGL(fcd_scene_minmax_fold_kernel, dim3(4 * C + 1), dim3(FCD_WAVE), 0, st, (const float*)parts,
                     (const unsigned long long*)counts, blocks, C, out, count);
  FCD_LAUNCH_CHECK("fcd_scene_minmax");
  return FCD_OK;
}
