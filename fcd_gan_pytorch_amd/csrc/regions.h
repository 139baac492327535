// Index arithmetic of csrc/regions.hip, kept apart so that a plain host program can drive every rule the kernels rely on
// (neighbour predicate, slice predicate, clamp rule, tile-to-pixel mapping) without a GPU: all of it is __host__ __device__
// and free of HIP types.  A host compiler that is not hipcc sees the qualifiers as nothing.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#define FCD_HD __host__ __device__ static inline

// The labelling tile: 64 columns (one lane per column, one wave instruction per row) x 16 rows = 1024 pixels = 4 KB of LDS.
enum { kRegTileW = 64, kRegTileH = 16, kRegTilePix = kRegTileW * kRegTileH };
// The ranking chunk: 1024 consecutive pixels of the raster, one workgroup of 256 threads x 4 pixels.
enum { kRegChunk = 1024 };

struct RegGeom {
  int H, W;
  int slice_h, slice_w;      // 0, 0: one slice
  int conn;                  // 1: 4 neighbours, 2: 8 neighbours
};

FCD_HD int reg_tiles_x(int W) { return (W + kRegTileW - 1) / kRegTileW; }
FCD_HD int reg_tiles_y(int H) { return (H + kRegTileH - 1) / kRegTileH; }
FCD_HD long long reg_tiles(int H, int W) { return (long long)reg_tiles_x(W) * reg_tiles_y(H); }
FCD_HD long long reg_chunks(int H, int W) { return ((long long)H * W + kRegChunk - 1) / kRegChunk; }

// tile t (row-major over the tile grid), local pixel l = ty * 64 + tx  ->  scene (y, x); false when outside the scene.
// Local order and raster order agree inside a tile, so the smallest local index of a set is its smallest pixel index too.
FCD_HD bool reg_tile_pixel(const RegGeom& g, long long t, int l, int* y, int* x) {
  const int tx = reg_tiles_x(g.W);
  *y = (int)(t / tx) * kRegTileH + l / kRegTileW;
  *x = (int)(t % tx) * kRegTileW + l % kRegTileW;
  return *y < g.H && *x < g.W;
}
FCD_HD long long reg_pixel_index(const RegGeom& g, int y, int x) { return (long long)y * g.W + x; }
FCD_HD long long reg_tile_of(const RegGeom& g, int y, int x) {
  return (long long)(y / kRegTileH) * reg_tiles_x(g.W) + x / kRegTileW;
}

// (y, x) and (ny, nx) lie in one slice: BuildingProcess labels every slice on its own
FCD_HD bool reg_same_slice(const RegGeom& g, int y, int x, int ny, int nx) {
  if (g.slice_h <= 0) return true;
  return y / g.slice_h == ny / g.slice_h && x / g.slice_w == nx / g.slice_w;
}
// column x begins a slice (a row run never continues across it)
FCD_HD bool reg_slice_starts_at(const RegGeom& g, int x) { return g.slice_w > 0 && x % g.slice_w == 0; }

// The four neighbours a pixel is united with (the other four unite with it): k = 0 left, 1 up-left, 2 up, 3 up-right.
FCD_HD int reg_nb_dy(int k) { return k == 0 ? 0 : -1; }
FCD_HD int reg_nb_dx(int k) { return k == 3 ? 1 : k == 2 ? 0 : -1; }
// (y, x) is joined to its k-th neighbour when that one lies in the scene, the connectivity has it (the diagonals k = 1, 3 need
// connectivity 2) and no slice border runs between the two.  Says nothing about either pixel being foreground.
FCD_HD bool reg_joined(const RegGeom& g, int y, int x, int k, int* ny, int* nx) {
  *ny = y + reg_nb_dy(k);
  *nx = x + reg_nb_dx(k);
  if (*ny < 0 || *nx < 0 || *nx >= g.W) return false;
  if ((k & 1) && g.conn != 2) return false;
  return reg_same_slice(g, y, x, *ny, *nx);
}

// Growth and clamp of one box, OSCDProcess.py:68-71 / BuildingProcess.py:140-143: against the slice that holds the box's first
// corner, intersected with the scene; without slices against the scene.  box = min_y, min_x, max_y, max_x (half-open).
FCD_HD int reg_grow_lo(int lo, int e, int bound) { return (long long)lo - e > bound ? lo - e : bound; }
FCD_HD int reg_grow_hi(int hi, int e, int bound) { return (long long)hi + e < bound ? hi + e : bound; }
FCD_HD void reg_grow_box(const RegGeom& g, const int32_t box[4], int e, int out[4]) {
  int y0 = 0, x0 = 0, y1 = g.H, x1 = g.W;
  if (g.slice_h > 0) {
    y0 = box[0] / g.slice_h * g.slice_h;
    x0 = box[1] / g.slice_w * g.slice_w;
    y1 = (long long)y0 + g.slice_h < g.H ? y0 + g.slice_h : g.H;
    x1 = (long long)x0 + g.slice_w < g.W ? x0 + g.slice_w : g.W;
  }
  out[0] = reg_grow_lo(box[0], e, y0);
  out[1] = reg_grow_lo(box[1], e, x0);
  out[2] = reg_grow_hi(box[2], e, y1);
  out[3] = reg_grow_hi(box[3], e, x1);
}

// Row runs: ``fg`` = the foreground bits of 64 consecutive columns starting at column x0 (bit c = column x0 + c), ``brk`` = the
// bits of the columns that begin a slice.  Bit c of the result is set where a run starts; the run of a foreground column c
// starts at the highest set bit at or below c.
FCD_HD unsigned long long reg_run_starts(unsigned long long fg, unsigned long long brk) { return fg & (~(fg << 1) | brk | 1ull); }
FCD_HD int reg_run_start_of(unsigned long long starts, int c) {
  const unsigned long long s = starts & ((2ull << c) - 1ull);          // c = 63: 2 << 63 wraps to 0, - 1 = all ones
  return 63 - __builtin_clzll(s);
}
