/* Internal declarations shared by the kernel TU and the C-ABI TU. */
#ifndef MIBAYER_INTERNAL_H
#define MIBAYER_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mibayer {

constexpr int kNumXcd = 8;      /* MI355X: 8 XCDs, block b is dispatched to XCD b % 8 */

/* Unsigned 32-bit division by a launch-time constant without a divide
 * (Granlund & Montgomery): 3 scalar instructions instead of the ~100-instruction
 * 64-bit division sequence the compiler emits for `a / b` with runtime b. */
struct FastDiv {
  uint32_t d;                   /* the divisor          */
  uint32_t mul;                 /* magic multiplier     */
  uint32_t sh1, sh2;            /* post-shifts          */
};

inline FastDiv make_fastdiv (uint32_t d)
{
  FastDiv f;
  f.d = d ? d : 1;
  uint32_t l = 0;               /* ceil (log2 d) */
  while (l < 32 && (1ull << l) < f.d)
    l++;
  f.mul = (uint32_t) ((((1ull << l) - f.d) << 32) / f.d + 1);
  f.sh1 = l < 1 ? l : 1;
  f.sh2 = l > 0 ? l - 1 : 0;
  return f;
}

__host__ __device__ inline uint32_t fastdiv (uint32_t n, const FastDiv &f)
{
  const uint32_t t = (uint32_t) (((unsigned long long) n * f.mul) >> 32);
  return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

/* XCD-aware block -> tile map, identical on host and device.
 *
 * Blocks are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8) and
 * each XCD has a private 4 MiB L2.  With the identity map horizontally adjacent
 * tiles land on different XCDs, so every tile's left/right halo dword drags a
 * full 128-byte line of its neighbour through the fabric a second time
 * (measured: L2->fabric reads = 2.0x the algorithmic bytes for 256-px tiles).
 *
 * The band map hands XCD k whole tile rows: tile row R (counted through the
 * batch, R = frame * tiles_y + ty) belongs to XCD (R / band) % 8, and an XCD
 * walks its rows left to right.  band = ceil (tile_rows / 8) gives every XCD one
 * contiguous chunk of the batch; band = 0 selects the identity map.
 * Everything is 32-bit (grids are < 2^31 blocks) and division-free. */
struct TileMap {
  FastDiv tiles_x;              /* tiles per tile row                           */
  FastDiv tiles_y;              /* tile rows per frame                          */
  FastDiv per_group;            /* band * tiles_x                               */
  uint32_t tile_rows;           /* tile rows of this launch (nframes * tiles_y, or
                                   the rows of one horizontal band of one frame) */
  uint32_t row0;                /* first tile row of this launch (0 unless a band) */
  int band;                     /* tile rows per XCD band; 0 = identity map     */
};

struct TileId {
  uint32_t row;                 /* tile row in the batch (TileMap.row0 included) */
  uint32_t tx;
  bool valid;
};

__host__ __device__ inline TileId block_to_tile (uint32_t block, const TileMap &m)
{
  TileId t;
  if (m.band <= 0) {
    t.row = fastdiv (block, m.tiles_x);
    t.tx = block - t.row * m.tiles_x.d;
  } else {
    const uint32_t xcd = block & (kNumXcd - 1);
    const uint32_t i = block / kNumXcd;         /* i-th block of this XCD */
    const uint32_t group = fastdiv (i, m.per_group);
    const uint32_t in_group = i - group * m.per_group.d;
    const uint32_t r_local = fastdiv (in_group, m.tiles_x);
    t.tx = in_group - r_local * m.tiles_x.d;
    t.row = (group * kNumXcd + xcd) * (uint32_t) m.band + r_local;
  }
  t.valid = t.row < m.tile_rows;
  t.row += m.row0;
  return t;
}

/* linear tile index (row * tiles_x + tx) -> TileId, for the persistent arm */
__host__ __device__ inline TileId linear_to_tile (uint32_t tile, const TileMap &m)
{
  TileId t;
  t.row = fastdiv (tile, m.tiles_x);
  t.tx = tile - t.row * m.tiles_x.d;
  t.valid = t.row < m.tile_rows;
  t.row += m.row0;
  return t;
}

inline long long grid_blocks_for (int tiles_x, long long tile_rows, int band)
{
  if (band <= 0)
    return tile_rows * tiles_x;
  const long long group_rows = (long long) kNumXcd * band;
  const long long groups = (tile_rows + group_rows - 1) / group_rows;
  return groups * group_rows * tiles_x;
}

inline TileMap make_tile_map (int tiles_x, int tiles_y, long long tile_rows,
    int band, long long row0 = 0)
{
  TileMap m;
  m.tiles_x = make_fastdiv ((uint32_t) tiles_x);
  m.tiles_y = make_fastdiv ((uint32_t) tiles_y);
  m.per_group = make_fastdiv ((uint32_t) (band > 0 ? band : 1)
      * (uint32_t) tiles_x);
  m.tile_rows = (uint32_t) tile_rows;
  m.row0 = (uint32_t) row0;
  m.band = band;
  return m;
}

constexpr int kMaxList = 16;    /* frames of one list launch (mibayer_process_device_list) */

/* Kernel arguments (passed by value -> SGPRs). */
struct KParams {
  const uint8_t *src;
  uint8_t *dst;
  unsigned long long src_frame_bytes;
  unsigned long long dst_frame_bytes;
  int width;
  int height;
  int src_stride;
  int dst_stride;
  int wlimit4;                  /* ROUND_UP_4(width): last readable column + 1 */
  int dn_last;                  /* source row standing in for row `height`     */
  TileMap map;
  int start_sleep;              /* s_sleep(1) iterations before a workgroup's first load */
  uint32_t sel[4];              /* v_perm_b32 selectors of output pixel 0..3   */
  int swap_rows;                /* 1 for grbg / gbrg                           */
  /* list launch: frame f is read at src_list[f] and written at dst_list[f] (frames that are
   * separate allocations, e.g. one GstBuffer each) instead of src / dst + f * frame bytes */
  int nlist;
  const uint8_t *src_list[kMaxList];
  uint8_t *dst_list[kMaxList];
};

/* frame index is wave-uniform: the table look-up is a scalar load from the kernel arguments */
__device__ __forceinline__ const uint8_t *frame_src (const KParams &p, uint32_t frame)
{
  return p.nlist ? p.src_list[frame] : p.src + frame * p.src_frame_bytes;
}

__device__ __forceinline__ uint8_t *frame_dst (const KParams &p, uint32_t frame)
{
  return p.nlist ? p.dst_list[frame] : p.dst + frame * p.dst_frame_bytes;
}

struct Variant {
  const char *name;
  int tile_w;                   /* pixels */
  int tile_h;                   /* rows   */
  int threads;
  int band;                     /* XCD band map: tile rows per band; 0 = identity, -1 = one
                                   contiguous chunk per XCD */
  int persistent;               /* 1: `fast` is a persistent kernel launched with a
                                   CU-count-sized grid that loops over the tiles */
  void (*fast) (KParams);       /* W%16==0, 16-byte aligned rows both sides */
  void (*generic) (KParams);    /* any even W >= 4, 4-byte aligned rows     */
  /* generic geometry whose output rows start off the 64-byte sector grid: every wave-store starts on a
   * 64- / 128-byte boundary (per-row lane shift, mibayer_kernels.hip); needs 8-byte aligned output rows.
   * nullptr: the variant has no such arm */
  void (*aligned64) (KParams);
  void (*aligned128) (KParams);
};

int variant_count ();
const Variant &variant (int id);
int resolve_variant (int id, int width);        /* 0 ("auto") -> a concrete id */
/* batch-class default (variant id 1-3, band) of a frame width with a measured winner the rules miss; false: none */
bool known_width_plan (int width, int *variant, int *band);
/* "auto" for a launch of one frame: the production shape whose grid needs the fewest rounds of `slots` workgroups */
int frame_class_variant (int width, int height, int slots);
/* the plain-store (write-back) arm of a production shape (ids 1-3), for output rows that start off a
 * 64-byte sector; any other id is returned unchanged */
int plain_store_twin (int id);
int hybrid_store_twin (int id);                 /* 1 -> 7, 2 -> 8, 3 -> 9: the hybrid store policy */
int production_shape_of (int id);               /* the inverse of both: 4, 7 -> 1; 5, 8 -> 2; 6, 9 -> 3 */

/* rgb2bayer (reference gst/bayer/gstrgb2bayer.c:230-278) */
struct R2BParams {
  const uint8_t *src;           /* 4 B/pixel */
  uint8_t *dst;                 /* 1 B/pixel mosaic */
  unsigned long long src_frame_bytes;
  unsigned long long dst_frame_bytes;
  int width;
  int height;
  int src_stride;
  int dst_stride;
  int out_dwords;               /* ROUND_UP_4(width) / 4 */
  long long total_rows;         /* nframes * height */
  int band;                     /* XCD band map (see block_to_tile); -1 = one chunk per XCD */
  int start_sleep;              /* s_sleep(1) iterations before the first load (tuning) */
  TileMap map;                  /* filled by launch_rgb2bayer: tiles = R rows x 1024 px */
  FastDiv div_height;
  uint32_t sel_lo[2];           /* v_perm selectors per row parity: pixels 0,1 */
  uint32_t sel_hi[2];           /*                                  pixels 2,3 */
  /* launch shape (tuning; every combination is bit-exact):
   *   flat_k  > 0: the flat kernel, the batch as one linear sequence of 4-pixel items (16 B in, one dword out),
   *                flat_k groups per thread kept in flight; 0: the tile kernel (rows x 1024 px per block)
   *   flat_px   4: one item per group (dword store), 8: two adjacent items per group (two 16-byte loads, one
   *                8-byte store; needs an even number of dwords per row and 8-byte aligned destination rows)
   *   flat_ld   1: nt hint on the loads (the input is read exactly once)
   *   rows      rows per block of the tile kernel (2, 4, 8, 16)                                             */
  int flat_k, flat_px, flat_ld, rows;
  FastDiv div_out_dwords;       /* filled by launch_rgb2bayer (flat kernel) */
  uint32_t item0, item_end;     /* first / one-past-last 4-pixel item of this launch (flat kernel) */
  /* list launch (flat kernel): frame f is read at src_list[f] and written at dst_list[f] -- frames that are
   * separate allocations, one GstBuffer each.  Every frame takes a whole number of blocks (blocks_per_frame), so
   * the frame index is block-uniform and the table look-up a scalar load from the kernel arguments */
  int nlist;
  FastDiv div_blocks_per_frame;
  const uint8_t *src_list[kMaxList];
  uint8_t *dst_list[kMaxList];
};
/* rows [row0, row0 + nrows) of the batch (nrows < 0: all); row0 must be a multiple of 16 */
hipError_t launch_rgb2bayer (const R2BParams &p, bool vec16, hipStream_t stream,
    long long row0 = 0, long long nrows = -1);
/* one launch over p.nlist (<= kMaxList) separately allocated frames (p.src_list / p.dst_list); needs the flat
 * kernel (p.flat_k > 0); dst8: every destination 8-byte aligned (two items per store allowed) */
hipError_t launch_rgb2bayer_list (const R2BParams &p, bool vec16, bool dst8, hipStream_t stream);

/* The strip kernels.  bayer2rgb on deep samples (MIBAYER_FLAG_SRC_BITS / MIBAYER_FLAG_DST_16BIT): 16-bit-word mosaics
 * of 10-16 significant bits, and/or 16-bit-per-channel output; Malvar-He-Cutler (MIBAYER_FLAG_MHC) and the fused colour
 * stage (MIBAYER_FLAG_COLOUR) on the same arguments.  One wave owns a strip of 256 pixels x kStripRows rows ("chunk") */
constexpr int kStripRows = 16;
struct DeepParams {
  const uint8_t *src;
  uint8_t *dst;
  unsigned long long src_frame_bytes;
  unsigned long long dst_frame_bytes;
  int width;
  int height;
  int src_stride;
  int dst_stride;
  int dn_last;                  /* source row standing in for row `height` */
  int swap_rows;                /* 1 for grbg / gbrg */
  uint32_t in_sel;              /* v_perm selector on a source dword: identity or a byte swap per 16-bit word */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  int out_shift;                /* 16-bit out: left shift (16 - bits); 8-bit out: right shift (bits - 8) */
  uint32_t sel[4];              /* 8-bit out: v_perm selectors of output pixel k (mibayer_plan_selectors) */
  uint32_t sel16[2][2];         /* 16-bit out: [pixel parity][dword of the pixel], over {R'B' word, G word} */
  /* the site map and the values' range: bayer2rgb_mhc_kernel and both arms of bayer2rgb_colour_kernel */
  int green_odd;                /* green sites of row 0 are at odd columns (bggr, rggb) */
  int red_odd;                  /* red sites are in odd rows (bggr, gbrg) */
  int vmax;                     /* 2^depth - 1 */
  uint32_t sel_cgd[2][2];       /* [row: 0 = its non-green colour is R, 1 = B][output dword], v_perm selectors over
                                   {x = [C, G], y = [D, 0]} at output depth; 4-byte output uses [.][0] only */
  int px3;                      /* 8-bit channels only: 3-byte pixels (MIBAYER_FLAG_DST_24BIT), the selectors those of
                                   RGBx / BGRx and byte 3 dropped at the store (store_strip8) */
  int planar;                   /* 8-bit channels only, 0 or 0x100 | p0 | p1 << 2 | p2 << 4: three planes instead of
                                   pixels (MIBAYER_FLAG_DST_PLANAR, store_planes8), plane k = rows [k * height,
                                   (k + 1) * height) of dst_stride bytes (the plane pitch is height * dst_stride).
                                   p0, p1, p2 = the plane index of the kernel's three operands: R, G, B (MHC, colour
                                   stage); the bilinear kernel's R', G, B' -- R' / B' swapped for rggb / gbrg like its
                                   selectors, which are not used.  One field: the colour kernel has no scalar register
                                   to spare */
  /* filled by launch_strip */
  int groups;                   /* 4-pixel groups per row = ceil (width / 4) */
  FastDiv div_tiles_x;          /* 256-pixel strips per row */
  FastDiv div_chunks;           /* chunks per frame */
  uint32_t chunk0;              /* first chunk of the launch (host-path bands) */
  uint32_t nwaves;              /* chunks of the launch x strips */
  int nlist;                    /* list launch: frame f at src_list[f] / dst_list[f] */
  const uint8_t *src_list[kMaxList];
  uint8_t *dst_list[kMaxList];
};
/* Fused colour stage (MIBAYER_FLAG_COLOUR, bayer2rgb_colour_kernel): black level, Q12 matrix, tone curve on the
 * demosaiced native-depth values, before the output conversion.  The matrix entry m is split as m = hi * 4096 + lo
 * (hi = m >> 12 in [-16, 15], lo = m & 4095): sum (m v) = 4096 * sum (hi v) + sum (lo v) with v <= 65535, so both sums
 * fit 32 bits (< 2^22 and < 2^30) and (acc + 2048) >> 12 = sum (hi v) + ((sum (lo v) + 2048) >> 12) exactly. */
struct ColourStage {
  int has_tone;
  int black[3];                 /* R, G, B */
  int m_hi[9], m_lo[9];         /* row-major, output channel x input channel */
  uint32_t tone[257];
};
/* the kernel's argument: the deep kernel's (first, so that its list tables keep their offsets) + the stage; the tone
 * table travels with every launch, so a launch keeps the table it was enqueued with */
struct ColourParams {
  DeepParams d;
  int mhc;                      /* demosaic by the MHC filters (else the deep path's bilinear closed form) */
  int in8, out16;
  ColourStage s;
};
/* which strip kernel: Malvar-He-Cutler or the bilinear closed form, 8-bit mosaic or 16-bit words, 8- or 4-byte output
 * pixels */
struct StripKind { bool mhc, in8, out16; };
/* One launch of a strip kernel over chunks [chunk0, chunk0 + nchunks) of the batch (nchunks < 0: all of p.nlist frames,
 * or of `nframes`).  stage = NULL: bayer2rgb_deep_kernel / bayer2rgb_mhc_kernel of the kind; bilinear 8-bit mosaic to
 * 4-byte pixels is refused (the production kernels serve it; to 3-byte pixels, p.px3, or planes, p.planar, it is the
 * deep kernel's).
 * Otherwise bayer2rgb_colour_kernel with that stage: one
 * kernel for both demosaic methods and all four input / output combinations (uniform run-time branches) */
hipError_t launch_strip (const DeepParams &p, StripKind kind, const ColourStage *stage, int nframes, hipStream_t stream,
    long long chunk0 = 0, long long nchunks = -1);

/* Half-size demosaic (MIBAYER_FLAG_HALF, bayer2rgb_half_kernel; include/mibayer.h, group `half`): one output pixel per
 * CFA quad, pointwise.  A lane owns 4 output pixels (8 source columns of two rows), a wave a strip of kHalfWavePixels
 * output pixels x kHalfRows output rows, a workgroup four such waves in launch order.  One kernel: sample width, output
 * format and the colour stage are uniform run-time branches. */
constexpr int kHalfLanePixels = 4;
constexpr int kHalfWavePixels = 64 * kHalfLanePixels;
constexpr int kHalfGroupPixels = 4 * kHalfWavePixels;   /* a workgroup's four waves side by side, when the row is that long */
constexpr int kHalfRows = 4;
/* the kernel's argument: the strip kernels' in OUTPUT geometry (d.width = OW, d.height = OH, so that the strip stores'
 * plane pitch and row ends are the output's; d.src_stride, d.in_sel, d.mask2, d.out_shift, d.green_odd, d.red_odd,
 * d.vmax, d.sel_cgd[0], d.px3, d.planar as the colour kernel reads them) + the colour kernel's switches and stage */
struct HalfParams {
  DeepParams d;
  int in8, out16;
  int colour;                   /* run the stage (MIBAYER_FLAG_COLOUR) */
  ColourStage s;
};
/* one launch over `nframes` frames (or the p.d.nlist frames of the list); stage = NULL: no colour stage */
hipError_t launch_half (const DeepParams &p, bool in8, bool out16, const ColourStage *stage, int nframes,
    hipStream_t stream);

/* Mosaic zone statistics (mosaic_stats_kernel; include/mibayer.h, group `stats`): read-only over the mosaic, one kernel
 * for both sample widths and byte orders (uniform run-time branches) */
constexpr int kStatsSegRows = 64;       /* rows a workgroup walks; even, so a segment starts on an even row */
constexpr int kStatsMaxZones = 64;
struct StatsParams {
  const uint8_t *src;
  unsigned long long src_frame_bytes;
  unsigned long long *stats;    /* nframes x zones_y x zones_x zones of 64 bytes: sum[4] (64-bit), count[4], clipped[4] */
  int width, height, src_stride;
  int in8;                      /* 8-bit mosaic: four samples per dword; else two 16-bit words */
  uint32_t in_sel;              /* v_perm selector on a source dword: identity or a byte swap per 16-bit word */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  uint32_t lo, hi;
  int zones_x, zones_y;
  int ch;                       /* rows of a zone */
  FastDiv div_cw;               /* pixels of a zone */
  /* filled by launch_stats */
  int row_dwords;               /* dwords of a row that hold columns < width (the last one may hold two columns past it) */
  int segs;                     /* segments of kStatsSegRows rows per zone row */
  FastDiv div_strips;           /* workgroups (4 waves x 64 dwords) per row */
};
/* one launch over `nframes` frames; p.stats must have been zeroed on the stream before */
hipError_t launch_stats (const StatsParams &p, int nframes, hipStream_t stream);

/* Mosaic histogram (mosaic_hist_kernel; include/mibayer.h, group `hist`): read-only over the mosaic, one kernel for both
 * sample widths and byte orders (uniform run-time branches) */
constexpr int kHistReps = 8;            /* LDS replicas of the [site][bin] table, one per lane & 7 */
constexpr int kHistAhead = 8;           /* dword loads in flight per lane = depth of the row loop */
constexpr int kHistMaxRows = 256;       /* rows a workgroup walks at most (256 KiB read per 4 KiB merged), even */
constexpr int kHistMinRows = 16;        /* ... and at least, when the launch is too small to fill the device otherwise */
constexpr int kHistSpread = 512;        /* workgroups a launch is spread over before the rows per workgroup grow */
struct HistParams {
  const uint8_t *src;
  unsigned long long src_frame_bytes;
  uint32_t *hist;               /* nframes x [site 4][bin 256] */
  int src_stride;
  int in8;                      /* 8-bit mosaic: four samples per dword; else two 16-bit words */
  uint32_t in_sel;              /* v_perm selector on a source dword: identity or a byte swap per 16-bit word */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  int shift;                    /* depth - 8 */
  int x0, x1, y0, y1;           /* the window: columns [x0, x1), rows [y0, y1) */
  /* filled by launch_hist */
  int g0, g1;                   /* dwords of a row that hold columns of the window */
  int seg_rows;                 /* rows a workgroup walks, even */
  FastDiv div_strips;           /* workgroups (4 waves x 64 dwords) per row of the window */
};
/* one launch over `nframes` frames; p.hist must have been zeroed on the stream before */
hipError_t launch_hist (const HistParams &p, int nframes, hipStream_t stream);

/* Mosaic focus statistics (mosaic_focus_kernel; include/mibayer.h, group `focus`): read-only over the mosaic, the launch
 * geometry of mosaic_stats_kernel (segments of kStatsSegRows rows of one zone row) and the five-row window of
 * mosaic_dpc_kernel, one kernel per sample width, both byte orders */
struct FocusParams {
  const uint8_t *src;
  unsigned long long src_frame_bytes;
  unsigned long long *focus;    /* nframes x zones_y x zones_x zones of 96 bytes: h[4], v[4] (64-bit), nh[4], nv[4] */
  int width, height, src_stride;
  int in8;                      /* 8-bit mosaic: four samples per dword; else two 16-bit words */
  uint32_t in_sel;              /* v_perm selector on a source dword: identity or a byte swap per 16-bit word */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  uint32_t thr;                 /* a response counts when |r| >= thr; <= 2 max */
  int zones_x, zones_y;
  int ch;                       /* rows of a zone */
  FastDiv div_cw;               /* pixels of a zone */
  /* filled by launch_focus */
  int row_dwords;               /* dwords of a row that hold columns < width (the last one may hold two columns past it) */
  int segs;                     /* segments of kStatsSegRows rows per zone row */
  FastDiv div_strips;           /* workgroups (4 waves x 64 dwords) per row */
};
/* one launch over `nframes` frames; p.focus must have been zeroed on the stream before */
hipError_t launch_focus (const FocusParams &p, int nframes, hipStream_t stream);

/* Lens shading correction (mosaic_shade_kernel; include/mibayer.h, group `shading`): a pointwise pass over the mosaic,
 * in place or into a second mosaic of the same sample format, one kernel per sample width, both byte orders */
constexpr int kShadeAhead = 8;          /* dword loads in flight per lane = depth of the row loop; even */
constexpr int kShadeMaxRows = 64;       /* rows a workgroup walks at most, even */
constexpr int kShadeMinRows = 16;       /* ... and at least, when the launch is too small to fill the device otherwise */
constexpr int kShadeSpread = 1024;      /* workgroups a launch is spread over before the rows per workgroup grow */
constexpr int kShadeMaxNodes = 129;     /* per direction */
struct ShadeParams {
  const uint8_t *src;
  uint8_t *dst;                 /* may be src */
  unsigned long long src_frame_bytes, dst_frame_bytes;
  const uint16_t *table;        /* device memory: [site 4][ny][nx], Q12 */
  int width, height, src_stride, dst_stride;
  int in8;                      /* 8-bit mosaic: four samples per dword; else two 16-bit words */
  uint32_t in_sel;              /* v_perm selector on a dword: identity or a byte swap per 16-bit word (its own inverse) */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  int vmax;                     /* 2^depth - 1 */
  int kx, ky;                   /* log2 of a cell's width / height, 2 .. 8 */
  int nx, ny;                   /* nodes per row / column of a site's plane */
  int black[4];                 /* per site */
  int y0, y1;                   /* rows [y0, y1) */
  /* filled by launch_shade */
  int row_dwords;               /* dwords of a row that hold columns < width (the last one may hold two columns past it) */
  int seg_rows;                 /* rows a workgroup walks, even */
  FastDiv div_strips;           /* workgroups (4 waves x 64 dwords) per row */
};
/* one launch over rows [p.y0, p.y1) of `nframes` frames */
hipError_t launch_shade (const ShadeParams &p, int nframes, hipStream_t stream);

/* Defective pixel correction (mosaic_dpc_kernel, mosaic_dpc_list_kernel; include/mibayer.h, group `dpc`): a 5 x 5
 * same-site neighbourhood pass from one mosaic into a second one of the same sample format, never in place */
constexpr int kDpcMaxRows = 64;         /* rows a workgroup walks at most */
constexpr int kDpcMinRows = 16;         /* ... and at least, when the launch is too small to fill the device otherwise */
constexpr int kDpcSpread = 1024;        /* workgroups a launch is spread over before the rows per workgroup grow */
struct DpcParams {
  const uint8_t *src;
  uint8_t *dst;                 /* never src */
  unsigned long long src_frame_bytes, dst_frame_bytes;
  const uint32_t *list;         /* device memory: (x, y) pairs sorted by (y, x); the entries [list_lo, list_hi) lie in
                                 * rows [y0, y1) (the caller bisects) */
  int list_lo, list_hi;
  int width, height, src_stride, dst_stride;
  int in8;                      /* 8-bit mosaic: four samples per dword; else two 16-bit words */
  uint32_t in_sel;              /* v_perm selector on a dword: identity or a byte swap per 16-bit word (its own inverse) */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  int hot, cold;                /* thresholds, -1 = off */
  int y0, y1;                   /* rows [y0, y1) */
  /* filled by launch_dpc */
  int row_dwords;               /* dwords of a row that hold columns < width (the last one may hold two columns past it) */
  int seg_rows;                 /* rows a workgroup walks */
  FastDiv div_strips;           /* workgroups (4 waves x 64 dwords) per row */
};
/* rows [p.y0, p.y1) of `nframes` frames: the detection and copy pass, then -- behind it on the same stream -- the
 * listed defects of those rows */
hipError_t launch_dpc (const DpcParams &p, int nframes, hipStream_t stream);

/* Noise reduction (mosaic_nr_kernel; include/mibayer.h, group `nr`): a sigma filter over the 24 same-site neighbours at
 * +-2 and +-4, from one mosaic into a second one of the same sample format, never in place */
constexpr int kNrMaxRows = 64;          /* rows a workgroup walks at most */
constexpr int kNrMinRows = 16;          /* ... and at least, when the launch is too small to fill the device otherwise */
constexpr int kNrSpread = 1024;         /* workgroups a launch is spread over before the rows per workgroup grow */
struct NrParams {
  const uint8_t *src;
  uint8_t *dst;                 /* never src */
  unsigned long long src_frame_bytes, dst_frame_bytes;
  int width, height, src_stride, dst_stride;    /* width >= 6 and even, height >= 5 */
  int in8;                      /* 8-bit mosaic: four samples per dword; else two 16-bit words */
  uint32_t in_sel;              /* v_perm selector on a dword: identity or a byte swap per 16-bit word (its own inverse) */
  uint32_t mask2;               /* sample mask in both halves of a dword */
  int shift;                    /* depth - 4: a sample's curve interval is S >> shift */
  int y0, y1;                   /* rows [y0, y1) */
  int lut[16][2];               /* per interval k: curve[k], curve[k + 1] - curve[k] */
  /* filled by launch_nr */
  uint32_t rcp[26];             /* ceil (2^32 / (2 cnt)), cnt = 1 .. 25 */
  int row_dwords;               /* dwords of a row that hold columns < width (the last one may hold two columns past it) */
  int seg_rows;                 /* rows a workgroup walks */
  FastDiv div_strips;           /* workgroups (4 waves x 64 dwords) per row */
};
/* one launch over rows [p.y0, p.y1) of `nframes` frames; rows up to four outside that range are read */
hipError_t launch_nr (const NrParams &p, int nframes, hipStream_t stream);

/* a kernel that only waits, `ms` milliseconds (drills: mibayer_internal_stall) */
hipError_t launch_stall (int ms, hipStream_t stream);

/* synthetic mosaic generator kernel launcher */
hipError_t launch_fill_synthetic (uint8_t *d_buf, int width, int height,
    int stride, unsigned long long frame_bytes, uint32_t first_frame,
    int nframes, uint32_t seed, hipStream_t stream);

}  /* namespace mibayer */
#endif
