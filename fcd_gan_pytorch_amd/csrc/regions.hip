// Region supervision maps from a change map, on the device: threshold, label the connected components, take their bounding
// boxes, grow every box and paint it -- what the reference does offline with skimage (OSCDProcess.py:56-73,
// BuildingProcess.py:127-145).  Integer bookkeeping only; HBM- and atomic-bound, no matrix work.
//
// LABELLING is union-find on a parent plane that lives in the caller's ``labels`` buffer: parent[i] <= i for every foreground
// pixel i (background holds -1), entries are lowered only by integer atomicMin, so every find walks a strictly descending chain
// and ends after at most i steps whatever the other workgroups do meanwhile -- there is no spin-wait, no flag, no cooperative
// launch and no grid-wide barrier; the phases are separated by KERNEL boundaries:
//   1. reg_local_kernel    one 64 x 16 tile per workgroup, in LDS: row runs by ballot (every pixel starts at the first pixel of its
//                          run, so chains are short), then one union per pair of overlapping / diagonal runs of adjacent rows;
//                          the tile-local roots go out as global pixel indices.
//   2. reg_merge_kernel    unites across tile edges: left, up and, for connectivity 2, both upper diagonals (corners included).
//                          The parent plane is read with device-scope atomic loads: a stale parent is still an ancestor, so a
//                          stale read would be correct, but it lengthens the chain.
//   3. reg_flatten_kernel  every pixel points at its root; counts the roots (parent[i] == i) of every 1024-pixel chunk of the raster.
//   4. reg_scan_kernel     exclusive scan of the chunk counts (one workgroup), total = K.
//   5. reg_assign_kernel   root i gets rank = roots before it in raster order + 1, stored as -1 - rank (<= -2).
//   6. reg_resolve_kernel  background -> 0, root -> its rank, every other pixel -> the rank of its root.
// The root of a set is its smallest pixel index, so the ranks number the components in raster order of their first pixel
// (scipy.ndimage.label's numbering), without a host read-back and without an order-dependent counter: two runs agree bit for bit.
// The index arithmetic (tile mapping, neighbour and slice predicates, clamp rule) is in regions.h, host-callable.
#include "common.h"
#include "regions.h"

constexpr int kRegBlock = 256, kRegWaves = kRegBlock / FCD_WAVE;
constexpr int kRegMaxGrid = 1 << 20;          // more tiles / chunks than that go round the grid-stride loops
constexpr int kRegMergeBlock = 128;           // 64 top-row + 15 left-column + 15 right-column pixels of a tile
constexpr int kRegScanBlock = 1024;
constexpr int kRegBoxGroup = 256, kRegBoxBatch = 4;   // segments the box scan keeps together / takes per wave and trip

static inline unsigned reg_grid(long long units) { return (unsigned)std::min<long long>(std::max<long long>(units, 1), kRegMaxGrid); }

// ---- union-find ---------------------------------------------------------------------------------------------------------
// GLOBAL: the plane is shared by every workgroup -- relaxed device-scope atomic loads (served by L2, never by a CU's L1).
// LDS: the tile's own plane.
template <bool GLOBAL>
__device__ __forceinline__ int uf_load(const int* p, int i) {
  if (GLOBAL) return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *(const volatile int*)(p + i);
}
// strictly descending: v < i at every step; a value that is not a smaller pixel index (a root, or anything unexpected) ends it
template <bool GLOBAL>
__device__ __forceinline__ int uf_find(const int* p, int i) {
  for (;;) {
    const int v = uf_load<GLOBAL>(p, i);
    if (v >= i || v < 0) return i;
    i = v;
  }
}
// The larger root is hung under the smaller one.  When another thread lowered p[a] first, atomicMin leaves min(old, b) there and
// the loop goes on uniting old with b, so no link is lost; max(a, b) falls with every trip.
template <bool GLOBAL>
__device__ __forceinline__ void uf_union(int* p, int a, int b) {
  for (;;) {
    a = uf_find<GLOBAL>(p, a);
    b = uf_find<GLOBAL>(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + a, b);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ bool reg_foreground(const void* __restrict__ map, int type, long long i, double thresh) {
  double v;
  if (type == FCD_SAMPLE_U8) v = (double)((const uint8_t*)map)[i];
  else if (type == FCD_SAMPLE_U16) v = (double)((const uint16_t*)map)[i];
  else v = (double)((const float*)map)[i];
  return v > thresh;                                         // NaN > t is false: background
}

// ---- 1. tile-local labelling ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRegBlock) void reg_local_kernel(const void* __restrict__ map, int type, double thresh, RegGeom g,
                                                              long long tiles, int* __restrict__ parent) {
  __shared__ int lp[kRegTilePix];
  const int lane = threadIdx.x & (FCD_WAVE - 1), w = threadIdx.x >> 6;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {       // block-uniform trip count: every wave reaches the barriers
    // A: row runs.  Wave w takes rows w, w + 4, ...; lane = column.
    for (int r = w; r < kRegTileH; r += kRegWaves) {
      const int l = r * kRegTileW + lane;
      int y, x;
      const bool in = reg_tile_pixel(g, t, l, &y, &x);
      const bool fg = in && reg_foreground(map, type, reg_pixel_index(g, y, x), thresh);
      const unsigned long long m = __ballot(fg);
      const unsigned long long brk = __ballot(in && reg_slice_starts_at(g, x));
      lp[l] = fg ? r * kRegTileW + reg_run_start_of(reg_run_starts(m, brk), lane) : -1;
    }
    __syncthreads();
    // B: unions with the row above.  Two runs of adjacent rows that overlap do so first at a column where one of them starts, so
    // only those columns unite; a diagonal matters only where the pixel straight above is background (otherwise the upper row's
    // own run already holds the diagonal pixel).  ``lp[..] >= 0`` (foreground) never changes, whatever the unions do.
    for (int r = w; r < kRegTileH; r += kRegWaves) {
      const int l = r * kRegTileW + lane;
      int y, x, ny, nx;
      if (r == 0 || !reg_tile_pixel(g, t, l, &y, &x) || lp[l] < 0) continue;
      const bool up = reg_joined(g, y, x, 2, &ny, &nx) && lp[l - kRegTileW] >= 0;
      if (up) {
        const bool left_run = lane > 0 && lp[l - 1] >= 0 && reg_joined(g, y, x, 0, &ny, &nx);
        const bool up_left_run = lane > 0 && lp[l - kRegTileW - 1] >= 0 && reg_joined(g, y - 1, x, 0, &ny, &nx);
        if (!left_run || !up_left_run) uf_union<false>(lp, l, l - kRegTileW);
      } else {
        if (lane > 0 && reg_joined(g, y, x, 1, &ny, &nx) && lp[l - kRegTileW - 1] >= 0) uf_union<false>(lp, l, l - kRegTileW - 1);
        if (lane < kRegTileW - 1 && reg_joined(g, y, x, 3, &ny, &nx) && lp[l - kRegTileW + 1] >= 0)
          uf_union<false>(lp, l, l - kRegTileW + 1);
      }
    }
    __syncthreads();
    // C: every pixel of the scene is written -- the global index of its tile-local root, or -1
    for (int r = w; r < kRegTileH; r += kRegWaves) {
      const int l = r * kRegTileW + lane;
      int y, x, ry, rx;
      if (!reg_tile_pixel(g, t, l, &y, &x)) continue;
      int out = -1;
      if (lp[l] >= 0) {
        reg_tile_pixel(g, t, uf_find<false>(lp, l), &ry, &rx);
        out = (int)reg_pixel_index(g, ry, rx);
      }
      parent[reg_pixel_index(g, y, x)] = out;
    }
    __syncthreads();                                                // lp is reused by the next tile
  }
}

// ---- 2. merge across tile edges ----------------------------------------------------------------------------------------------
// Items of a tile: 0..63 its top row, 64..78 its left column below the corner, 79..93 its right column below the corner.  Every
// item looks at its four earlier neighbours and unites with those that lie in ANOTHER tile.
__global__ __launch_bounds__(kRegMergeBlock) void reg_merge_kernel(RegGeom g, long long tiles, int* __restrict__ parent) {
  const int it = threadIdx.x;
  int l;
  if (it < kRegTileW) l = it;
  else if (it < kRegTileW + kRegTileH - 1) l = (it - kRegTileW + 1) * kRegTileW;
  else if (it < kRegTileW + 2 * (kRegTileH - 1)) l = (it - (kRegTileW + kRegTileH - 1) + 1) * kRegTileW + kRegTileW - 1;
  else return;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    int y, x, ny, nx;
    if (!reg_tile_pixel(g, t, l, &y, &x)) continue;
    const int i = (int)reg_pixel_index(g, y, x);
    if (uf_load<true>(parent, i) < 0) continue;
    const bool up = reg_joined(g, y, x, 2, &ny, &nx) && uf_load<true>(parent, (int)reg_pixel_index(g, ny, nx)) >= 0;
    for (int k = 0; k < 4; ++k) {
      if ((k & 1) && up) continue;                                  // the upper row's run holds the diagonal pixel already
      if (!reg_joined(g, y, x, k, &ny, &nx) || reg_tile_of(g, ny, nx) == t) continue;
      const int n = (int)reg_pixel_index(g, ny, nx);
      if (uf_load<true>(parent, n) >= 0) uf_union<true>(parent, i, n);
    }
  }
}

// ---- 3. flatten + count the roots of every chunk ---------------------------------------------------------------------------
// Chunk c = pixels c * 1024 ... ; thread t takes pixels c * 1024 + j * 256 + t, j < 4: position j * 256 + t in the chunk.
__global__ __launch_bounds__(kRegBlock) void reg_flatten_kernel(int* __restrict__ parent, long long N, long long chunks,
                                                                int32_t* __restrict__ counts) {
  __shared__ int total;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int roots = 0;
    for (int j = 0; j < kRegChunk / kRegBlock; ++j) {
      const long long i = c * kRegChunk + j * kRegBlock + threadIdx.x;
      bool root = false;
      if (i < N) {
        const int v = uf_load<true>(parent, (int)i);
        if (v >= 0) {
          const int r = uf_find<true>(parent, (int)i);
          root = r == (int)i;
          // another walker may read this entry meanwhile: the old value and the root are both ancestors
          if (r != v) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      roots += __popcll(__ballot(root));
    }
    if ((threadIdx.x & (FCD_WAVE - 1)) == 0 && roots) atomicAdd(&total, roots);      // LDS, integer: order does not matter
    __syncthreads();
    if (threadIdx.x == 0) counts[c] = total;
    __syncthreads();
  }
}

// ---- 4. exclusive scan of the chunk counts, in place; *count = their sum -----------------------------------------------------
__global__ __launch_bounds__(kRegScanBlock) void reg_scan_kernel(int32_t* __restrict__ counts, long long n, int32_t* __restrict__ count) {
  __shared__ int wsum[kRegScanBlock / FCD_WAVE];
  const int lane = threadIdx.x & (FCD_WAVE - 1), w = threadIdx.x >> 6;
  int carry = 0;
  for (long long base = 0; base < n; base += kRegScanBlock) {
    const long long i = base + threadIdx.x;
    const int v = i < n ? counts[i] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < FCD_WAVE; o <<= 1) {
      const int u = __shfl_up(incl, o, FCD_WAVE);
      if (lane >= o) incl += u;
    }
    if (lane == FCD_WAVE - 1) wsum[w] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < kRegScanBlock / FCD_WAVE; ++k) {
      const int s = wsum[k];
      if (k < w) before += s;
      total += s;
    }
    if (i < n) counts[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
}

// ---- 5. ranks of the roots ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRegBlock) void reg_assign_kernel(int* __restrict__ parent, long long N, long long chunks,
                                                               const int32_t* __restrict__ offsets) {
  constexpr int kSlots = kRegChunk / FCD_WAVE;                      // one per 64 consecutive pixels of the chunk
  __shared__ int cnt[kSlots];
  const int lane = threadIdx.x & (FCD_WAVE - 1), w = threadIdx.x >> 6;
  for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
    bool root[kRegChunk / kRegBlock];
    unsigned long long m[kRegChunk / kRegBlock];
#pragma unroll
    for (int j = 0; j < kRegChunk / kRegBlock; ++j) {
      const long long i = c * kRegChunk + j * kRegBlock + threadIdx.x;
      root[j] = i < N && parent[i] == (int)i;
      m[j] = __ballot(root[j]);
      if (lane == 0) cnt[j * kRegWaves + w] = __popcll(m[j]);
    }
    __syncthreads();
    const int off = offsets[c];
#pragma unroll
    for (int j = 0; j < kRegChunk / kRegBlock; ++j) {
      if (!root[j]) continue;
      int before = __popcll(m[j] & ((1ull << lane) - 1ull));
      for (int k = 0; k < j * kRegWaves + w; ++k) before += cnt[k];
      parent[c * kRegChunk + j * kRegBlock + threadIdx.x] = -1 - (off + before + 1);
    }
    __syncthreads();
  }
}

// ---- 6. labels ---------------------------------------------------------------------------------------------------------------
// A thread writes its own entry only.  The entry of a root is -1 - rank until its own thread turns it into rank, so whichever of
// the two a reader meets it decodes the same number.
__global__ __launch_bounds__(kRegBlock) void reg_resolve_kernel(int* __restrict__ labels, long long N) {
  for (long long i = (long long)blockIdx.x * kRegBlock + threadIdx.x; i < N; i += (long long)gridDim.x * kRegBlock) {
    const int v = labels[i];
    int out = 0;
    if (v <= -2) {
      out = -1 - v;
    } else if (v >= 0) {
      const int x = uf_load<true>(labels, v);
      out = x < 0 ? -1 - x : x;
    }
    labels[i] = out;
  }
}

static bool reg_sample_type_ok(int t) { return t == FCD_SAMPLE_U8 || t == FCD_SAMPLE_U16 || t == FCD_SAMPLE_F32; }
static bool reg_slices_ok(int sh, int sw) { return (sh == 0 && sw == 0) || (sh > 0 && sw > 0); }

extern "C" size_t fcd_label_components_ws_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (long long)H * W > INT32_MAX) return 0;
  return (size_t)reg_chunks(H, W) * sizeof(int32_t);
}

extern "C" int fcd_label_components(const void* map, int sample_type, int H, int W, double thresh, int connectivity, int slice_h,
                                    int slice_w, int32_t* labels, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  FCD_CHECK_ARG(map && labels && count && H > 0 && W > 0, "fcd_label_components: bad arguments");
  FCD_CHECK_ARG((long long)H * W <= INT32_MAX, "fcd_label_components: %d x %d pixels, at most 2^31 - 1", H, W);
  FCD_CHECK_ARG(reg_sample_type_ok(sample_type), "fcd_label_components: sample type %d (0 uint8, 1 uint16, 2 float32)", sample_type);
  FCD_CHECK_ARG(connectivity == 1 || connectivity == 2, "fcd_label_components: connectivity %d (1: 4 neighbours, 2: 8 neighbours)",
                connectivity);
  FCD_CHECK_ARG(reg_slices_ok(slice_h, slice_w), "fcd_label_components: slice %d x %d (both 0, or both positive)", slice_h, slice_w);
  const size_t need = fcd_label_components_ws_bytes(H, W);
  FCD_CHECK_ARG(ws && ws_bytes >= need, "fcd_label_components: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const RegGeom g{H, W, slice_h, slice_w, connectivity};
  const long long N = (long long)H * W, tiles = reg_tiles(H, W), chunks = reg_chunks(H, W);
  const double sample = sample_type == FCD_SAMPLE_U8 ? 1.0 : sample_type == FCD_SAMPLE_U16 ? 2.0 : 4.0;
  FcdProfScope prof(FCD_K_MISC, st, 0.0, (double)N * (sample + 6 * 4.0));
  int32_t* counts = (int32_t*)ws;
  hipLaunchKernelGGL(reg_local_kernel, dim3(reg_grid(tiles)), dim3(kRegBlock), 0, st, map, sample_type, thresh, g, tiles, labels);
  hipLaunchKernelGGL(reg_merge_kernel, dim3(reg_grid(tiles)), dim3(kRegMergeBlock), 0, st, g, tiles, labels);
  hipLaunchKernelGGL(reg_flatten_kernel, dim3(reg_grid(chunks)), dim3(kRegBlock), 0, st, labels, N, chunks, counts);
  hipLaunchKernelGGL(reg_scan_kernel, dim3(1), dim3(kRegScanBlock), 0, st, counts, chunks, count);
  hipLaunchKernelGGL(reg_assign_kernel, dim3(reg_grid(chunks)), dim3(kRegBlock), 0, st, labels, N, chunks, (const int32_t*)counts);
  hipLaunchKernelGGL(reg_resolve_kernel, dim3(reg_grid(cdiv64(N, kRegBlock))), dim3(kRegBlock), 0, st, labels, N);
  FCD_LAUNCH_CHECK("fcd_label_components");
  return FCD_OK;
}

// ---- boxes ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRegBlock) void reg_boxes_init_kernel(int32_t* __restrict__ boxes, int K, int H, int W) {
  for (long long k = (long long)blockIdx.x * kRegBlock + threadIdx.x; k < K; k += (long long)gridDim.x * kRegBlock)
    ((int4*)boxes)[k] = make_int4(H, W, 0, 0);
}

// A wave takes kRegBoxBatch consecutive 64-column segments of the raster per trip, all their loads issued before the first is
// looked at.  Atomics are folded in three steps (Guideline 12): the lane at the head of a run of one label speaks for the run; the
// runs that carry the label of the segment's FIRST run -- all of them where a large component fills the segment with many runs --
// are reduced over the wave and their first lane speaks for them; and a speaker asks for an atomic only where the box it reads
// (device-scope loads; what it reads can only be looser than the true box, as minima only fall and maxima only rise) does not hold
// its columns and row yet.  The segments are taken in groups from both ends of the raster inwards, so that the box of a component
// that spans the scene is wide after the first waves and the rest only read it.  Integer min / max: the result does not depend
// on the order of arrival.
__device__ __forceinline__ void reg_box_segment(int L, int y, int x0, int lane, int K, int32_t* __restrict__ boxes) {
  const int prev = __shfl_up(L, 1, FCD_WAVE);
  const bool change = lane == 0 || prev != L;
  const unsigned long long cm = __ballot(change);
  const bool head = change && L > 0 && L <= K;
  const unsigned long long hm = __ballot(head);
  if (!hm) return;                                                                   // wave-uniform
  const unsigned long long later = cm & ~((2ull << lane) - 1ull);
  int lo = x0 + lane, hi = x0 + (later ? __builtin_ctzll(later) : FCD_WAVE);         // the run: columns lo .. hi - 1
  const int first = __builtin_ctzll(hm);
  const bool shared = head && L == __shfl(L, first, FCD_WAVE);
  if (hm & (hm - 1)) {                                                               // more than one run (wave-uniform)
    int slo = shared ? lo : INT32_MAX, shi = shared ? hi : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      slo = min(slo, __shfl_xor(slo, o, FCD_WAVE));
      shi = max(shi, __shfl_xor(shi, o, FCD_WAVE));
    }
    if (shared) { lo = slo; hi = shi; }
  }
  if (!head || (shared && lane != first)) return;
  int32_t* b = boxes + (long long)(L - 1) * 4;
  const int b0 = uf_load<true>(b, 0), b1 = uf_load<true>(b, 1), b2 = uf_load<true>(b, 2), b3 = uf_load<true>(b, 3);
  if (y < b0) atomicMin(b + 0, y);
  if (lo < b1) atomicMin(b + 1, lo);
  if (y + 1 > b2) atomicMax(b + 2, y + 1);
  if (hi > b3) atomicMax(b + 3, hi);
}

__global__ __launch_bounds__(kRegBlock) void reg_boxes_kernel(const int32_t* __restrict__ labels, int H, int W, int K,
                                                              long long units, int segs, int32_t* __restrict__ boxes) {
  const int lane = threadIdx.x & (FCD_WAVE - 1);
  const long long wave = (long long)blockIdx.x * kRegWaves + (threadIdx.x >> 6);
  const long long groups = (units + kRegBoxGroup - 1) / kRegBoxGroup;
  for (long long u = wave * kRegBoxBatch; u < groups * kRegBoxGroup; u += (long long)gridDim.x * kRegWaves * kRegBoxBatch) {
    // groups of 256 segments (64 KB of labels, read in raster order) in the order 0, last, 1, last - 1, ...: a bijection
    const long long grp = u / kRegBoxGroup;
    const long long v0 = ((grp & 1) ? groups - 1 - (grp >> 1) : (grp >> 1)) * kRegBoxGroup + u % kRegBoxGroup;
    int L[kRegBoxBatch], y[kRegBoxBatch], x0[kRegBoxBatch];
#pragma unroll
    for (int j = 0; j < kRegBoxBatch; ++j) {                  // a batch never straddles two groups: 256 is a multiple of the batch
      const long long v = v0 + j;
      y[j] = (int)(v / segs);
      x0[j] = (int)(v % segs) * FCD_WAVE;
      L[j] = v < units && x0[j] + lane < W ? labels[(long long)y[j] * W + x0[j] + lane] : 0;      // past the raster: background
    }
#pragma unroll
    for (int j = 0; j < kRegBoxBatch; ++j) reg_box_segment(L[j], y[j], x0[j], lane, K, boxes);
  }
}

extern "C" int fcd_component_boxes(const int32_t* labels, int H, int W, int K, int32_t* boxes, void* stream) {
  FCD_CHECK_ARG(labels && H > 0 && W > 0 && K >= 0 && (boxes || K == 0), "fcd_component_boxes: bad arguments");
  FCD_CHECK_ARG((long long)H * W <= INT32_MAX, "fcd_component_boxes: %d x %d pixels, at most 2^31 - 1", H, W);
  FCD_CHECK_ARG(K <= (long long)H * W, "fcd_component_boxes: %d components in %d x %d pixels", K, H, W);
  FCD_CHECK_ARG(((uintptr_t)boxes & 15) == 0, "fcd_component_boxes: the boxes must be 16-byte aligned");
  if (K == 0) return FCD_OK;
  hipStream_t st = (hipStream_t)stream;
  const int segs = cdiv(W, FCD_WAVE);
  const long long units = (long long)H * segs;
  FcdProfScope prof(FCD_K_MISC, st, 0.0, (double)H * W * 4.0 + (double)K * 32.0);
  hipLaunchKernelGGL(reg_boxes_init_kernel, dim3(reg_grid(cdiv64(K, kRegBlock))), dim3(kRegBlock), 0, st, boxes, K, H, W);
  hipLaunchKernelGGL(reg_boxes_kernel, dim3(reg_grid(cdiv64(cdiv64(units, kRegBoxGroup) * kRegBoxGroup, kRegWaves * kRegBoxBatch))), dim3(kRegBlock), 0, st, labels, H, W, K, units,
                     segs, boxes);
  FCD_LAUNCH_CHECK("fcd_component_boxes");
  return FCD_OK;
}

// ---- paint -----------------------------------------------------------------------------------------------------------------------
// blockIdx.x strides over the boxes, blockIdx.y and the four waves over the rows of the grown box, the lanes along a row.  Boxes
// that overlap store the same byte.  The grown box is cut to the scene once more, so that no box, whatever it holds, leaves it.
__global__ __launch_bounds__(kRegBlock) void reg_paint_kernel(const int32_t* __restrict__ boxes, int K, RegGeom g, int expand,
                                                              uint8_t* __restrict__ region) {
  const int lane = threadIdx.x & (FCD_WAVE - 1), w = threadIdx.x >> 6;
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    const int4 b4 = ((const int4*)boxes)[k];
    const int32_t b[4] = {b4.x, b4.y, b4.z, b4.w};
    if (b[0] < 0 || b[1] < 0 || b[0] >= b[2] || b[1] >= b[3] || b[2] > g.H || b[3] > g.W) continue;     // not a box of this scene
    int o[4];
    reg_grow_box(g, b, expand, o);
    const int y0 = max(o[0], 0), x0 = max(o[1], 0), y1 = min(o[2], g.H), x1 = min(o[3], g.W);
    for (int y = y0 + blockIdx.y * kRegWaves + w; y < y1; y += gridDim.y * kRegWaves) {
      uint8_t* __restrict__ row = region + (long long)y * g.W;
      for (int x = x0 + lane; x < x1; x += FCD_WAVE) row[x] = 255;
    }
  }
}

extern "C" int fcd_region_paint(const int32_t* boxes, int K, int H, int W, int expand, int slice_h, int slice_w, uint8_t* region,
                                void* stream) {
  FCD_CHECK_ARG(region && H > 0 && W > 0 && K >= 0 && (boxes || K == 0), "fcd_region_paint: bad arguments");
  FCD_CHECK_ARG((long long)H * W <= INT32_MAX, "fcd_region_paint: %d x %d pixels, at most 2^31 - 1", H, W);
  FCD_CHECK_ARG(expand >= 0, "fcd_region_paint: expand %d is negative", expand);
  FCD_CHECK_ARG(reg_slices_ok(slice_h, slice_w), "fcd_region_paint: slice %d x %d (both 0, or both positive)", slice_h, slice_w);
  FCD_CHECK_ARG(((uintptr_t)boxes & 15) == 0, "fcd_region_paint: the boxes must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  FcdProfScope prof(FCD_K_MISC, st, 0.0, (double)H * W + (double)K * 16.0);
  if (hipMemsetAsync(region, 0, (size_t)H * W, st) != hipSuccess) {
    fcd_set_error("fcd_region_paint: clearing the map failed");
    return FCD_ERR_LAUNCH;
  }
  if (K > 0) {
    // few boxes may be large: spread each over several workgroups; many boxes are small
    const int gx = std::min(K, 65535 * 16);
    const int gy = std::max(1, std::min(cdiv(H, kRegWaves), 2048 / K));
    const RegGeom g{H, W, slice_h, slice_w, 2};
    hipLaunchKernelGGL(reg_paint_kernel, dim3(gx, gy), dim3(kRegBlock), 0, st, boxes, K, g, expand, region);
  }
  FCD_LAUNCH_CHECK("fcd_region_paint");
  return FCD_OK;
}
