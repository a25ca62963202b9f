/*
 * bayer2rgb demosaic for MI355X (gfx950, CDNA4) -- device code.
 *
 * Replaces, in ONE fused kernel, the reference's per-row CPU loops
 *   gst_bayer2rgb_split_and_upsample_horiz   gst/bayer/gstbayer2rgb.c:354-381
 *   bayer_orc_horiz_upsample_unaligned        gst/bayer/gstbayerorc.orc:3-19
 *   bayer_orc_merge_{bg,gr}_{bgra,abgr,rgba,argb}   gstbayerorc.orc:43-248
 * and the frame loop around them, gst_bayer2rgb_process (gstbayer2rgb.c:387-451).
 *
 * Algorithm (all uint8, avg(a,b) = (a+b+1)>>1, the ORC `avgub`):
 *   for every source row y two lines are defined (reference :354-381)
 *     E_y[x] = S(y,x)                 x even      O_y[x] = S(y,x)                 x odd
 *            = avg(S(y,x-1),S(y,x+1)) x odd              = avg(S(y,x-1),S(y,x+1)) x even
 *     with the edge columns  O_y[0]=S(y,1), E_y[W-1]=S(y,W-2), O_y[W-2]=S(y,W-3)
 *   output row j uses rows u=up(j), j, d=dn(j) where up(0)=1 and dn(H-1)=H-4
 *   (the reference's 4-slot ring, :430-447), and with T = (j&1)^swap_rows
 *     T=0 (merge_bg): B'=E_j  R'=avg(O_u,O_d)  G = x even ? avg(avg(E_u,E_d),O_j) : O_j
 *     T=1 (merge_gr): B'=avg(E_u,E_d)  R'=O_j  G = x even ? E_j : avg(avg(O_u,O_d),E_j)
 *   R'/B' land on the r/b byte offsets (swapped for rggb/gbrg, :403-407), the
 *   remaining byte is 255.
 *
 * Mapping to the machine:
 *   - a lane owns 4 horizontally adjacent pixels = one source dword, so a wave64
 *     reads 256 contiguous bytes and writes 1 KiB contiguous bytes per row
 *     (global_store_dwordx4, every 128-byte line fully written by one instruction);
 *   - all arithmetic is 4-pixels-per-instruction packed bytes: v_lerp_u8 is
 *     exactly avgub on four bytes, v_alignbit_b32 builds the x-1 / x+1 neighbour
 *     dwords, v_bfi_b32 does the even/odd column select, v_perm_b32 interleaves
 *     R',G,B',255 into the output pixels (selectors are kernel arguments, so one
 *     kernel serves all 4 byte layouts and all 4 Bayer orders);
 *   - a workgroup stages its tile plus one halo row above and below (and one halo
 *     dword left and right) in LDS with 16-byte coalesced loads; each wave then
 *     marches down its rows with a 3-row sliding window of (E,O) in registers;
 *   - the x-1 / x+4 neighbour bytes come from the adjacent lanes through DPP
 *     wave shifts (no memory traffic); only lanes 0 and 63 take theirs from LDS;
 *   - blockIdx -> tile is XCD-aware (mibayer_internal.h: block_to_tile; tile_of gives the tile's frame and origin).
 * The tile kernels share TileShape (constants), tile_of, stage_rows_generic, edge_lines (the edge columns), march_rows
 * and store_two; see "what the tile kernels share" below.
 * The op is a pure HBM stream (1 B read + 4 B written per pixel, ~25 integer
 * ops per 4 pixels): no MFMA.
 */
#include "mibayer_internal.h"

#include <stdlib.h>
#include <type_traits>

namespace mibayer {

typedef uint32_t u32x4 __attribute__ ((ext_vector_type (4)));
typedef uint32_t u32x2 __attribute__ ((ext_vector_type (2)));
/* the same at dword alignment: all a gfx950 global load / store needs.  The generic paths (rows
 * that are not 16-byte aligned: width % 16 != 0, padded strides, odd pointers) move 16 bytes per
 * instruction through these instead of dword by dword */
typedef uint32_t u32x4_a4 __attribute__ ((ext_vector_type (4), aligned (4)));
typedef uint32_t u32x2_a4 __attribute__ ((ext_vector_type (2), aligned (4)));
typedef uint32_t u32x3_a4 __attribute__ ((ext_vector_type (3), aligned (4)));   /* a store writes 12 bytes */

/* ------------------------------------------------------------------------- */
/* packed-byte primitives                                                     */
/* ------------------------------------------------------------------------- */

/* four avgub at once */
template <bool INTRIN>
__device__ __forceinline__ uint32_t avg4 (uint32_t a, uint32_t b)
{
  if constexpr (INTRIN) {
    /* v_lerp_u8: per byte (a + b + (c & 1)) >> 1 */
    return __builtin_amdgcn_lerp (a, b, 0x01010101u);
  } else {
    return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu);
  }
}

/* ({hi,lo} >> (8*nbytes)) & 0xffffffff */
template <bool INTRIN>
__device__ __forceinline__ uint32_t funnel_bytes (uint32_t hi, uint32_t lo,
    int nbytes)
{
  if constexpr (INTRIN) {
    return __builtin_amdgcn_alignbit (hi, lo, 8 * nbytes);
  } else {
    return (uint32_t) ((((unsigned long long) hi << 32) | lo) >> (8 * nbytes));
  }
}

/* v_perm_b32: byte i of the result is byte sel[i] of {s0,s1} (0-3 = s1, 4-7 = s0),
 * 12 = 0x00, >= 13 = 0xff */
template <bool INTRIN>
__device__ __forceinline__ uint32_t perm4 (uint32_t s0, uint32_t s1,
    uint32_t sel)
{
  if constexpr (INTRIN) {
    return __builtin_amdgcn_perm (s0, s1, sel);
  } else {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t idx = (sel >> (8 * i)) & 0xffu, b;
      if (idx < 4)
        b = (s1 >> (8 * idx)) & 0xffu;
      else if (idx < 8)
        b = (s0 >> (8 * (idx - 4))) & 0xffu;
      else if (idx == 12)
        b = 0;
      else
        b = 0xffu;
      r |= b << (8 * i);
    }
    return r;
  }
}

/* (m & a) | (~m & b)  ->  v_bfi_b32 */
__device__ __forceinline__ uint32_t bsel (uint32_t m, uint32_t a, uint32_t b)
{
  return (m & a) | (~m & b);
}

constexpr uint32_t kEvenBytes = 0x00ff00ffu;

/* DPP wave shifts (gfx9 encodings).  Lanes whose source lane does not exist
 * keep `edge`. */
__device__ __forceinline__ uint32_t from_lane_below (uint32_t edge, uint32_t v)
{
  /* wave_shr:1 -- lane i receives lane i-1 */
  return (uint32_t) __builtin_amdgcn_update_dpp ((int) edge, (int) v, 0x138,
      0xf, 0xf, false);
}

__device__ __forceinline__ uint32_t from_lane_above (uint32_t edge, uint32_t v)
{
  /* wave_shl:1 -- lane i receives lane i+1 */
  return (uint32_t) __builtin_amdgcn_update_dpp ((int) edge, (int) v, 0x130,
      0xf, 0xf, false);
}

/* ------------------------------------------------------------------------- */
/* per-row horizontal lines, reference gstbayer2rgb.c:354-381                  */
/* ------------------------------------------------------------------------- */

struct Lines { uint32_t e, o; };

/* (E,O) of the four columns c = S[x0..x0+3] from their x-1 / x+1 neighbour windows lsh = S[x0-1..x0+2] and
 * rsh = S[x0+1..x0+4], with the frame's edge columns: the one place that states them.
 * first: x0 == 0.   last4: this lane holds columns W-4..W-1.   last2: it holds columns W-2..W-1 only. */
template <bool INTRIN>
__device__ __forceinline__ Lines edge_lines (uint32_t lsh, uint32_t c,
    uint32_t rsh, bool first, bool last4, bool last2)
{
  /* O[0] = S[1] (:361): make the left neighbour of column 0 equal S[1] */
  uint32_t lsh_first = (lsh & 0xffffff00u) | ((c >> 8) & 0xffu);
  lsh = first ? lsh_first : lsh;
  /* E[W-1] = S[W-2], O[W-2] = S[W-3] (:372-380): right neighbours of the last
   * two columns are replaced by their left neighbours */
  uint32_t t = lsh >> 16;                    /* [c1, c2, 0, 0] */
  uint32_t rsh_last = t | (t << 16);          /* [c1, c2, c1, c2] */
  rsh = last4 ? rsh_last : rsh;
  rsh = last2 ? lsh : rsh;                    /* [L, c0, -, -] */
  uint32_t a = avg4<INTRIN> (lsh, rsh);
  Lines r;
  r.e = bsel (kEvenBytes, c, a);
  r.o = bsel (kEvenBytes, a, c);
  return r;
}

/* c  = S[x0..x0+3], cl = dword left of it, cr = dword right of it.
 * lastmode: 1 = this lane holds columns W-4..W-1, 2 = columns W-2..W-1 only (generic geometries). */
template <bool INTRIN, bool GENERIC>
__device__ __forceinline__ Lines row_lines (uint32_t c, uint32_t cl,
    uint32_t cr, bool first, int lastmode)
{
  /* x-1 neighbours: [cl.3, c0, c1, c2];  x+1 neighbours: [c1, c2, c3, cr.0] */
  uint32_t lsh = funnel_bytes<INTRIN> (c, cl, 3);
  uint32_t rsh = funnel_bytes<INTRIN> (cr, c, 1);
  return edge_lines<INTRIN> (lsh, c, rsh, first, lastmode == 1, GENERIC && lastmode == 2);
}

/* ------------------------------------------------------------------------- */
/* vertical merge + interleave, reference gstbayerorc.orc:43-92                */
/* ------------------------------------------------------------------------- */

template <bool INTRIN>
__device__ __forceinline__ u32x4 merge_rows (const Lines &u, const Lines &c,
    const Lines &d, int type, const uint32_t (&sel)[4])
{
  uint32_t ve = avg4<INTRIN> (u.e, d.e);
  uint32_t vo = avg4<INTRIN> (u.o, d.o);
  uint32_t rq, bq, g;
  if (type == 0) {              /* merge_bg, orc:57-66 */
    bq = c.e;
    rq = vo;
    g = bsel (kEvenBytes, avg4<INTRIN> (ve, c.o), c.o);
  } else {                      /* merge_gr, orc:83-92 */
    bq = ve;
    rq = c.o;
    g = bsel (kEvenBytes, c.e, avg4<INTRIN> (vo, c.e));
  }
  /* [r0 b0 r1 b1], [r2 b2 r3 b3] */
  uint32_t m_lo = perm4<INTRIN> (rq, bq, 0x01050004u);
  uint32_t m_hi = perm4<INTRIN> (rq, bq, 0x03070206u);
  u32x4 px;
  px.x = perm4<INTRIN> (m_lo, g, sel[0]);
  px.y = perm4<INTRIN> (m_lo, g, sel[1]);
  px.z = perm4<INTRIN> (m_hi, g, sel[2]);
  px.w = perm4<INTRIN> (m_hi, g, sel[3]);
  return px;
}

/* the lane that holds the last two columns of a width % 4 == 2 frame writes two pixels, at dword alignment */
template <bool NT>
__device__ __forceinline__ void store_two (uint8_t *p, u32x4 px)
{
  u32x2 two;
  two.x = px.x;
  two.y = px.y;
  if constexpr (NT)
    __builtin_nontemporal_store (two, (u32x2_a4 *) p);
  else
    *(u32x2_a4 *) p = two;
}

/* ST = cache policy of the 16-byte output stores (the output is never re-read):
 * 0 plain, 1 nt (streaming hint), 2 sc1, 3 sc0 sc1 (write-through, line dropped
 * from the XCD L2), 4 nt sc1; + 8 = nt hint on the LDS kernel's row loads too,
 * + 16 = direct-to-LDS row loads */
template <int STLD, bool GENERIC>
__device__ __forceinline__ void store_pixels (uint8_t *p, u32x4 px,
    int lastmode)
{
  constexpr int ST = STLD & 7;  /* bit 3 = nt hint on the tile's row loads, bit 4 = direct-to-LDS loads */
  if constexpr (!GENERIC) {
    if constexpr (ST == 1 || ST == 5)         /* 5: the hybrid policy of generic geometries; aligned rows stream */
      __builtin_nontemporal_store (px, (u32x4 *) p);
    else if constexpr (ST == 2)
      asm volatile ("global_store_dwordx4 %0, %1, off sc1" :: "v" (p), "v" (px) : "memory");
    else if constexpr (ST == 3)
      asm volatile ("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v" (p), "v" (px) : "memory");
    else if constexpr (ST == 4)
      asm volatile ("global_store_dwordx4 %0, %1, off sc1 nt" :: "v" (p), "v" (px) : "memory");
    else
      *(u32x4 *) p = px;
  } else {
    /* rows start at dword alignment only: same 16-byte store, at that alignment; the lane that
     * holds the last two columns of a width % 4 == 2 frame writes two pixels (store_two) */
    if (lastmode != 2) {
      if constexpr (ST == 1)
        __builtin_nontemporal_store (px, (u32x4_a4 *) p);
      else
        *(u32x4_a4 *) p = px;
    } else {
      store_two<ST == 1> (p, px);
    }
  }
}

/* Store policy 5 ("hybrid"), generic geometries: output rows that start off the 128-byte line grid make every 1 KiB
 * wave-store begin and end inside a line that a neighbouring wave (or tile) completes.  Streaming (nt) stores push
 * such half-written lines out one half at a time and lose 4-11 points of HBM peak; write-back stores let the L2 put
 * the halves together but give up what nt gains on a pure output stream (3 points; profiles/r03_generic_path.log).
 * Here each lane picks by itself: nt when every line its 16 bytes touch lies completely inside this wave-store,
 * write-back for the one or two ragged lines at either end.  a7 = position of the lane's first byte in its line;
 * the wave-store covers bytes [-lane16, len - lane16) relative to it. */
__device__ __forceinline__ void store_pixels_hybrid (uint8_t *p, u32x4 px,
    int lastmode, int lane16, int len)
{
  const int a7 = (int) ((uint32_t) (uintptr_t) p & 127u);
  const int need = a7 > 112 ? 256 : 128;        /* the 16 bytes straddle a line boundary: both lines count */
  const bool inside = a7 <= lane16 && lane16 + need - a7 <= len;
  if (lastmode == 2) {
    store_two<false> (p, px);
  } else if (inside) {
    /* spelled out: the compiler folds an nt and a plain store of the same value under if / else into ONE plain store */
    asm volatile ("global_store_dwordx4 %0, %1, off nt" :: "v" (p), "v" (px) : "memory");
  } else {
    asm volatile ("global_store_dwordx4 %0, %1, off" :: "v" (p), "v" (px) : "memory");
  }
}

/* source row standing in for row y of the (virtually extended) frame:
 * up(0) = 1, dn(H-1) = dn_last (H-4, or 1 when H == 3) -- gstbayer2rgb.c:430-447 */
__device__ __forceinline__ int map_row (int y, int height, int dn_last)
{
  return y < 0 ? 1 : (y < height ? y : dn_last);
}

/* ------------------------------------------------------------------------- */
/* what the tile kernels share: shape, tile origin, generic staging, march      */
/* ------------------------------------------------------------------------- */
/* WX x WY waves per workgroup; a wave covers 256 px (64 lanes x 4 px) and marches
 * RPW rows.  Tile = (256*WX) x (WY*RPW) px, staged with one halo row above and below
 * in 16-byte chunks, TPR threads per row and RPP rows per pass.  An LDS row starts
 * with 12 B pad | left halo dword, the tile's bytes follow at MAIN; what lies right
 * of them (PITCH) is the kernel's own.
 * The helpers take the kernel arguments as `const KParams &__restrict__`: through a plain reference the compiler
 * loads the selectors and the geometry again after every row's stores. */
template <int WX, int WY, int RPW>
struct TileShape {
  static constexpr int NTHREADS = 64 * WX * WY;
  static constexpr int TW = 256 * WX;
  static constexpr int TR = WY * RPW;
  static constexpr int NROWS = TR + 2;
  static constexpr int MAIN = 16;
  static constexpr int TPR = TW / 16;
  static constexpr int RPP = NTHREADS / TPR;
  static constexpr int NPASS = (NROWS + RPP - 1) / RPP;
  static_assert (RPW % 2 == 0, "row parity is derived from the in-tile row");
};

/* a tile's frame and its first pixel in it */
struct Tile { const uint8_t *src; uint8_t *dst; int tile_x, tile_y; };

template <int TW, int TR>
__device__ __forceinline__ Tile tile_of (const KParams &__restrict__ p, TileId id)
{
  const uint32_t frame = fastdiv (id.row, p.map.tiles_y);
  const int ty = (int) (id.row - frame * p.map.tiles_y.d);
  Tile t;
  t.src = frame_src (p, frame);
  t.dst = frame_dst (p, frame);
  t.tile_x = (int) id.tx * TW;
  t.tile_y = ty * TR;
  return t;
}

/* Generic geometry: rows tile_y-1 .. tile_y+TR (through map_row) of the tile into LDS in the same 16-byte chunks as the
 * fast arm, loaded at dword alignment; the chunk that straddles the end of a row (width % 16 != 0) is read dword by
 * dword up to ROUND_UP_4(width), which the source stride always covers.  Chunks right of the frame are zeros */
template <class S, int PITCH>
__device__ __forceinline__ void stage_rows_generic (const KParams &__restrict__ p,
    const Tile t, int tid, uint8_t *lds)
{
  const int c = (tid % S::TPR) * 16;
  const int rr = tid / S::TPR;
  const int avail = p.wlimit4 - (t.tile_x + c);         /* readable bytes from this chunk on */
  u32x4 v[S::NPASS];
#pragma unroll
  for (int i = 0; i < S::NPASS; i++) {
    const int r = i * S::RPP + rr;
    const int y = t.tile_y - 1 + r;
    v[i] = (u32x4) (0u);
    if (r < S::NROWS && y <= p.height && avail > 0) {
      const uint8_t *g = t.src
          + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride
          + t.tile_x + c;
      if (avail >= 16) {
        v[i] = *(const u32x4_a4 *) g;
      } else {
        const uint32_t *q = (const uint32_t *) g;
        v[i].x = q[0];
        if (avail > 4) v[i].y = q[1];
        if (avail > 8) v[i].z = q[2];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < S::NPASS; i++) {
    const int r = i * S::RPP + rr;
    if (r < S::NROWS)
      *(u32x4 *) &lds[r * PITCH + S::MAIN + c] = v[i];
  }
}

/* A wave's march down its rows with a 3-row sliding window of (E,O).  lines_of (r): the lines of staged row r, r0 the
 * one that is up of the wave's first output row; that row is row y0 + r0 of the frame at dst, the lane's columns are
 * x0..x0+3 (active: inside the frame); store (out, px) writes the four pixels of a row that lies inside the frame */
template <int RPW, bool INTRIN, class LinesOf, class Store>
__device__ __forceinline__ void march_rows (const KParams &__restrict__ p, uint8_t *dst,
    int y0, int r0, int x0, bool active, LinesOf lines_of, Store store)
{
  Lines up = lines_of (r0);
  Lines cur = lines_of (r0 + 1);
  uint8_t *out = dst + (size_t) (y0 + r0) * p.dst_stride + (size_t) x0 * 4;
  const int nrows = p.height - (y0 + r0);       /* rows of this wave inside the frame */
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const Lines dn = lines_of (r0 + k + 2);
    const int type = (k & 1) ^ p.swap_rows;
    const u32x4 px = merge_rows<INTRIN> (up, cur, dn, type, p.sel);
    if (active && k < nrows)
      store (out, px);
    out += p.dst_stride;
    up = cur;
    cur = dn;
  }
}

/* ------------------------------------------------------------------------- */
/* LDS-staged tile kernel                                                      */
/* ------------------------------------------------------------------------- */
/* NEIGH: 0 = DPP wave shift, 1 = __shfl_up/down (ds_bpermute), 2 = LDS reads.   */
template <int WX, int WY, int RPW, int NEIGH, int ST, bool INTRIN,
    bool GENERIC>
__global__ void __launch_bounds__ (64 * WX * WY)
bayer2rgb_lds_kernel (KParams p)
{
  using S = TileShape<WX, WY, RPW>;
  /* LDS row: 12 B pad | left halo dword | TW bytes | right halo dword | 12 B pad */
  constexpr int PITCH = S::TW + 32;
  constexpr int MAIN = S::MAIN;

  __shared__ __attribute__ ((aligned (16))) uint8_t lds[S::NROWS * PITCH];

  const TileId id = block_to_tile (blockIdx.x, p.map);
  if (!id.valid)
    return;
  /* start delay: lets the store burst of the workgroup that just
   * retired on this CU drain before this one's loads reach the L2 (input-FIFO-full
   * cycles drop 5-9x, profiles/r01_delay_counters.md); +3..5 points of HBM
   * peak for the band / chunk block orders.  Measured alternatives that lost:
   * the same delay after the barrier or after the stores, a per-workgroup
   * stagger, lower occupancy (profiles/r01_sweep_start_delay.log). */
  for (int z = 0; z < p.start_sleep; z++)
    __builtin_amdgcn_s_sleep (1);
  const Tile t = tile_of<S::TW, S::TR> (p, id);
  const int tile_x = t.tile_x;
  const int tile_y = t.tile_y;
  const int tid = threadIdx.x;

  /* ---- stage rows tile_y-1 .. tile_y+TR (through map_row) into LDS ---------- */
  if constexpr (!GENERIC && (ST & 16) != 0) {
    /* experiment arm: direct global -> LDS loads (global_load_lds_dwordx4), no
     * staging registers and no ds_write pass.  The LDS destination of such a load
     * is wave-uniform base + lane * 16, so it needs one wave per 1 KiB tile row:
     * WX == 4.  Lanes right of the frame skip their load; what their LDS bytes
     * hold is never used (the last valid lane replaces its right neighbour). */
    static_assert (WX == 4, "one wave stages one 1024-px row");
    constexpr int RPP = S::NTHREADS / 64;    /* rows per pass = waves */
    constexpr int NPASS = (S::NROWS + RPP - 1) / RPP;
    const int c = (tid & 63) * 16;
    const int rr = tid >> 6;
#pragma unroll
    for (int i = 0; i < NPASS; i++) {
      const int r = i * RPP + rr;
      const int y = tile_y - 1 + r;
      if (r < S::NROWS && y <= p.height && tile_x + c < p.width) {
        const uint8_t *g = t.src
            + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride
            + tile_x + c;
        __builtin_amdgcn_global_load_lds (
            (const __attribute__ ((address_space (1))) void *) g,
            (__attribute__ ((address_space (3))) void *) &lds[r * PITCH + MAIN],
            16, 0, 0);
      }
    }
  } else if constexpr (!GENERIC) {
    const int c = (tid % S::TPR) * 16;
    const int rr = tid / S::TPR;
    u32x4 v[S::NPASS];
#pragma unroll
    for (int i = 0; i < S::NPASS; i++) {
      const int r = i * S::RPP + rr;
      const int y = tile_y - 1 + r;
      v[i] = (u32x4) (0u);
      if (r < S::NROWS && y <= p.height && tile_x + c < p.width) {
        const uint8_t *g = t.src
            + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride
            + tile_x + c;
        if constexpr ((ST & 8) != 0)
          v[i] = __builtin_nontemporal_load ((const u32x4 *) g);
        else
          v[i] = *(const u32x4 *) g;
      }
    }
#pragma unroll
    for (int i = 0; i < S::NPASS; i++) {
      const int r = i * S::RPP + rr;
      if (r < S::NROWS)
        *(u32x4 *) &lds[r * PITCH + MAIN + c] = v[i];
    }
  } else {
    stage_rows_generic<S, PITCH> (p, t, tid, lds);
  }
  /* halo dwords: column tile_x-4 and tile_x+TW of every staged row */
  for (int h = tid; h < 2 * S::NROWS; h += S::NTHREADS) {
    const int r = h >> 1;
    const int side = h & 1;
    const int y = tile_y - 1 + r;
    const int col = side ? tile_x + S::TW : tile_x - 4;
    uint32_t v = 0u;
    if (y <= p.height && col >= 0 && col < p.wlimit4)
      v = *(const uint32_t *) (t.src
          + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride + col);
    *(uint32_t *) &lds[r * PITCH + (side ? MAIN + S::TW : MAIN - 4)] = v;
  }
  __syncthreads ();

  /* ---- per-wave march -------------------------------------------------------- */
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wx = wave % WX;
  const int wy = wave / WX;
  const int xl = 256 * wx + 4 * lane;
  const int x0 = tile_x + xl;
  const bool first = (x0 == 0);
  const int lastmode = (x0 + 4 == p.width) ? 1
      : ((GENERIC && x0 + 2 == p.width) ? 2 : 0);
  const bool active = x0 < p.width;
  const uint8_t *lrow = &lds[MAIN + xl];
  /* lanes 0 / 63 take the neighbour that lives in another wave (or the halo) */
  const int edge_off = (lane == 0) ? -4 : 4;

  auto lines_of = [&](int r) -> Lines {
    const uint8_t *q = lrow + r * PITCH;
    const uint32_t c = *(const uint32_t *) q;
    uint32_t cl, cr;
    if constexpr (NEIGH == 2) {
      cl = *(const uint32_t *) (q - 4);
      cr = *(const uint32_t *) (q + 4);
    } else {
      const uint32_t edge = *(const uint32_t *) (q + edge_off);
      if constexpr (NEIGH == 0) {
        cl = from_lane_below (edge, c);
        cr = from_lane_above (edge, c);
      } else {
        cl = __shfl_up (c, 1);
        cr = __shfl_down (c, 1);
        cl = (lane == 0) ? edge : cl;
        cr = (lane == 63) ? edge : cr;
      }
    }
    return row_lines<INTRIN, GENERIC> (c, cl, cr, first, lastmode);
  };

  /* march_rows, spelled out: called through it the fast arms, which carry the headline number, compile to other code
   * than the measured one (4 instructions and 4 VGPRs fewer, not timed), so this kernel keeps the loop in its body */
  const int r0 = wy * RPW;      /* LDS row of up(first output row of this wave) */
  Lines up = lines_of (r0);
  Lines cur = lines_of (r0 + 1);
  uint8_t *out = t.dst + (size_t) (tile_y + r0) * p.dst_stride + (size_t) x0 * 4;
  const int nrows = p.height - (tile_y + r0);   /* rows of this wave inside the frame */
  /* bytes of a row this wave writes (store policy 5): 1 KiB, less for the wave that holds the end of the row */
  const int wave_left = 4 * (p.width - (tile_x + 256 * wx));
  const int wave_len = wave_left < 1024 ? wave_left : 1024;
#pragma unroll
  for (int k = 0; k < RPW; k++) {
    const Lines dn = lines_of (r0 + k + 2);
    const int type = (k & 1) ^ p.swap_rows;
    const u32x4 px = merge_rows<INTRIN> (up, cur, dn, type, p.sel);
    if (active && k < nrows) {
      if constexpr (GENERIC && (ST & 7) == 5)
        store_pixels_hybrid (out, px, lastmode, 16 * lane, wave_len);
      else
        store_pixels<ST, GENERIC> (out, px, lastmode);
    }
    out += p.dst_stride;
    up = cur;
    cur = dn;
  }
}

/* (E,O) of four columns whose source bytes start R bytes (0 or 2) behind the dword-aligned LDS address qa: the
 * column dword and its x-1 / x+1 neighbour windows all come out of the aligned dwords around it (for R = 2 out of
 * two of them), so no lane exchange and no wave-edge special case is needed.  EDGE: this wave holds the first column
 * of the frame, or its last ones */
template <int R, bool EDGE>
__device__ __forceinline__ Lines shifted_lines (const uint8_t *qa, int x, int width)
{
  const uint32_t d0 = *(const uint32_t *) qa;
  const uint32_t d1 = *(const uint32_t *) (qa + 4);
  uint32_t lsh, c, rsh;         /* columns x-1..x+2, x..x+3, x+1..x+4 */
  if constexpr (R == 0) {
    const uint32_t dm = *(const uint32_t *) (qa - 4);
    lsh = __builtin_amdgcn_alignbit (d0, dm, 24);
    c = d0;
    rsh = __builtin_amdgcn_alignbit (d1, d0, 8);
  } else {
    lsh = __builtin_amdgcn_alignbit (d1, d0, 8);
    c = __builtin_amdgcn_alignbit (d1, d0, 16);
    rsh = __builtin_amdgcn_alignbit (d1, d0, 24);
  }
  return edge_lines<true> (lsh, c, rsh, EDGE && x == 0, EDGE && x + 4 == width, EDGE && x + 2 == width);
}

/* ------------------------------------------------------------------------- */
/* LDS-staged tile kernel, sector-aligned stores (generic geometries)          */
/* ------------------------------------------------------------------------- */
/* Output rows that do not start on a 64-byte sector (dst_stride % 64 != 0: every width % 16 != 0, e.g. 4056-,
 * 3838-, 1366-px frames).  In the kernel above a lane owns the SAME four columns in every row, so the 1 KiB a wave
 * stores per row starts wherever the row starts: each wave-store ends in a partial sector that a neighbouring wave
 * (or workgroup, or XCD) completes later.  Here the lane -> column map is shifted PER ROW instead: output row j
 * starts at address a_j = dst + j * dst_stride, s_j = ((-a_j) mod ALIGN) / 4 pixels, and lane l of wave wx of tile tx
 * converts columns  tile_x + 256 wx + 4 l + s_j ...+3  of that row.  Its 16-byte store then sits at
 * a_j + 4 s_j + 1024 (..) + 16 l: every wave-store is one 1 KiB run that starts on an ALIGN-byte boundary.  What is
 * left over is written once per row, by the first wave of the row: the s_j < ALIGN/4 columns in front of the first
 * boundary (the "head", at most ALIGN - 8 bytes); the row's ragged end is the last active lanes of the last tile.
 *
 * The price is arithmetic, not memory: the three source rows of an output row are looked up at that row's own
 * shift, so the (E,O) lines of a source row are built three times (once per output row that uses it) instead of
 * once -- ~45 instead of ~25 VALU instructions per 4 pixels, still a fraction of what the CUs have to spare on this
 * stream; waves that hold no frame edge in a row (all but the first and last of a row) run without the edge-column
 * selects.  A lane's column dword and both neighbour windows come out of the two or three ALIGNED LDS dwords around
 * them through v_alignbit_b32 (unaligned ds_reads were measured 2x slower), so the shifted arm needs no lane
 * exchange at all.  The tile carries ALIGN/4 + 4 more source columns on its right for it.
 *
 * Needs even shifts (a_j % 8 == 0 for every row: dst, dst_stride and the frame pitch multiples of 8); anything
 * else keeps the GENERIC arm of the kernel above.  Same arithmetic, bit-exact (tests/test_gpu_parity.py). */
template <int WX, int WY, int RPW, int ST, int ALIGN>
__global__ void __launch_bounds__ (64 * WX * WY)
bayer2rgb_lds_aligned_kernel (KParams p)
{
  using S = TileShape<WX, WY, RPW>;
  constexpr int SMAX = ALIGN / 4;               /* shifts are 0, 2, .. SMAX - 2 pixels */
  /* LDS row: 12 B pad | left halo dword | TW bytes | RIGHT bytes.  The last lane of the tile at the largest shift
   * reads its right neighbour dword at bytes TW - 4 + (SMAX - 2) + 4 .. + 7 */
  constexpr int RIGHT = (SMAX + 4 + 15) & ~15;
  constexpr int NRIGHT = (SMAX + 4) / 4;        /* dwords staged right of the tile */
  constexpr int PITCH = 16 + S::TW + RIGHT;
  static_assert (ALIGN == 64 || ALIGN == 128, "a sector or an L2 line");

  __shared__ __attribute__ ((aligned (16))) uint8_t lds[S::NROWS * PITCH];

  const TileId id = block_to_tile (blockIdx.x, p.map);
  if (!id.valid)
    return;
  for (int z = 0; z < p.start_sleep; z++)
    __builtin_amdgcn_s_sleep (1);
  const Tile t = tile_of<S::TW, S::TR> (p, id);
  const int tile_x = t.tile_x;
  const int tile_y = t.tile_y;
  const int tid = threadIdx.x;

  /* ---- stage rows tile_y-1 .. tile_y+TR, columns tile_x-4 .. tile_x+TW+4*NRIGHT-1 ---------- */
  {
    stage_rows_generic<S, PITCH> (p, t, tid, lds);
    /* halo dwords: one left of the tile, NRIGHT right of it */
    for (int h = tid; h < (1 + NRIGHT) * S::NROWS; h += S::NTHREADS) {
      const int r = h / (1 + NRIGHT);
      const int k = h - r * (1 + NRIGHT);
      const int y = tile_y - 1 + r;
      const int off = k == 0 ? -4 : S::TW + 4 * (k - 1);
      const int col = tile_x + off;
      uint32_t hv = 0u;
      if (y <= p.height && col >= 0 && col < p.wlimit4)
        hv = *(const uint32_t *) (t.src
            + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride + col);
      *(uint32_t *) &lds[r * PITCH + S::MAIN + off] = hv;
    }
  }
  __syncthreads ();

  /* ---- per-wave rows: no sliding window here.  A row's shift moves the lane -> column map, so the three source
   * rows of every output row are rebuilt at that row's own shift (by design, see above) and march_rows does not fit */
  const int wave = __builtin_amdgcn_readfirstlane (tid >> 6);
  const int lane = tid & 63;
  const int wx = wave % WX;
  const int wy = wave / WX;
  const int xl = 256 * wx + 4 * lane;   /* column inside the tile, before the row's shift */
  const int wave_x0 = tile_x + 256 * wx;
  const int r0 = wy * RPW;
  const int nrows = p.height - (tile_y + r0);   /* rows of this wave inside the frame */
  const bool head_wave = (id.tx == 0 && wx == 0);
  const uint8_t *lrow = &lds[r0 * PITCH + S::MAIN + xl];

  /* one output row of this wave at shift s: convert, store */
  auto shifted_row = [&](auto rtag, auto etag, const uint8_t *qa, int x, int type, uint8_t *row, int lim) {
    constexpr int R = decltype (rtag)::value;
    constexpr bool EDGE = decltype (etag)::value;
    const Lines up = shifted_lines<R, EDGE> (qa, x, p.width);
    const Lines cur = shifted_lines<R, EDGE> (qa + PITCH, x, p.width);
    const Lines dn = shifted_lines<R, EDGE> (qa + 2 * PITCH, x, p.width);
    const u32x4 px = merge_rows<true> (up, cur, dn, type, p.sel);
    uint8_t *out = row + (size_t) x * 4;
    if constexpr (!EDGE) {
      store_pixels<ST, false> (out, px, 0);
    } else {
      /* lim: one past the last column this pass may write (the frame width, or the first boundary for the head) */
      if (x + 4 <= lim)
        *(u32x4_a4 *) out = px;
      else if (x + 2 == lim)
        store_two<false> (out, px);
    }
  };
  using R0 = std::integral_constant<int, 0>;
  using R2 = std::integral_constant<int, 2>;

#pragma unroll
  for (int k = 0; k < RPW; k++) {
    if (k >= nrows)
      break;
    uint8_t *row = t.dst + (size_t) (tile_y + r0 + k) * p.dst_stride;
    const int s = (int) (((0u - (uint32_t) (uintptr_t) row) & (uint32_t) (ALIGN - 1)) >> 2);
    const int type = (k & 1) ^ p.swap_rows;
    const uint8_t *qa = lrow + k * PITCH + (s & ~3);
    const int wave_x = wave_x0 + s;     /* first column of this wave in this row */
    const int x = wave_x + 4 * lane;
    if (wave_x > 0 && wave_x + 256 < p.width) {
      /* no frame edge inside this wave: every lane converts and stores four pixels */
      if (s & 2)
        shifted_row (R2 (), std::false_type (), qa, x, type, row, 0);
      else
        shifted_row (R0 (), std::false_type (), qa, x, type, row, 0);
    } else {
      if (s & 2)
        shifted_row (R2 (), std::true_type (), qa, x, type, row, p.width);
      else
        shifted_row (R0 (), std::true_type (), qa, x, type, row, p.width);
    }
    /* the head of the row: columns 0 .. s-1 in front of the first boundary, at the natural (unshifted) lane map */
    if (head_wave && s > 0)
      shifted_row (R0 (), std::true_type (), lrow + k * PITCH, 4 * lane, type, row, s < p.width ? s : p.width);
  }
}

#ifdef MIBAYER_LAB
/* ------------------------------------------------------------------------- */
/* direct kernel: no LDS, every wave streams its own strip                     */
/* ------------------------------------------------------------------------- */
/* Experiment arm (same arithmetic): rows come straight from global memory, the
 * wave-edge lanes fetch their neighbour dword with a second, 2-lane load.      */
template <int WX, int WY, int RPW, int ST, bool INTRIN, bool GENERIC>
__global__ void __launch_bounds__ (64 * WX * WY)
bayer2rgb_direct_kernel (KParams p)
{
  using S = TileShape<WX, WY, RPW>;

  const TileId id = block_to_tile (blockIdx.x, p.map);
  if (!id.valid)
    return;
  const Tile t = tile_of<S::TW, S::TR> (p, id);
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wx = wave % WX;
  const int wy = wave / WX;
  const int x0 = t.tile_x + 256 * wx + 4 * lane;
  const int yb = t.tile_y + wy * RPW;
  const bool first = (x0 == 0);
  const int lastmode = (x0 + 4 == p.width) ? 1
      : ((GENERIC && x0 + 2 == p.width) ? 2 : 0);
  const bool active = x0 < p.width;
  const bool readable = x0 < p.wlimit4;
  const int xe = (lane == 0) ? x0 - 4 : x0 + 4;
  const bool edge_lane = (lane == 0 || lane == 63) && xe >= 0
      && xe < p.wlimit4;

  uint32_t c[RPW + 2], e[RPW + 2];
#pragma unroll
  for (int r = 0; r < RPW + 2; r++) {
    const int y = yb - 1 + r;
    c[r] = 0u;
    e[r] = 0u;
    if (y <= p.height) {
      const uint8_t *row = t.src
          + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride;
      if (readable)
        c[r] = *(const uint32_t *) (row + x0);
      if (edge_lane)
        e[r] = *(const uint32_t *) (row + xe);
    }
  }

  auto lines_of = [&](int r) -> Lines {
    const uint32_t cl = from_lane_below (e[r], c[r]);
    const uint32_t cr = from_lane_above (e[r], c[r]);
    return row_lines<INTRIN, GENERIC> (c[r], cl, cr, first, lastmode);
  };

  march_rows<RPW, INTRIN> (p, t.dst, yb, 0, x0, active, lines_of, [&](uint8_t *out, u32x4 px) {
    store_pixels<ST, GENERIC> (out, px, lastmode);
  });
}

/* ------------------------------------------------------------------------- */
/* persistent, double-buffered form of the LDS kernel (experiment arm)          */
/* ------------------------------------------------------------------------- */
/* One workgroup per CU slot loops over its share of the tiles; the global loads
 * of tile n+1 are issued before tile n is computed and stored, so the HBM read
 * latency hides under the store phase instead of under other workgroups
 * (Little's-law check: the per-tile kernel keeps ~25 of 32 waves resident and
 * they spend 57 % of their life parked on memory, profiles/r01_sq_counters.md).
 * Fast path only (W % 16 == 0, aligned rows); same arithmetic, same stores.
 * MEASURED SLOWER (-12 points): one barrier per tile makes all 8 waves of a
 * workgroup load, then store, in lock step, while independent small workgroups
 * keep the memory pipes evenly fed.  Kept as an A/B arm, not used by "auto".  */
template <int WX, int WY, int RPW, int ST>
__global__ void __launch_bounds__ (64 * WX * WY)
bayer2rgb_persist_kernel (KParams p)
{
  using S = TileShape<WX, WY, RPW>;
  constexpr int PITCH = S::TW + 32;
  constexpr int MAIN = S::MAIN;
  static_assert (2 * S::NROWS <= S::NTHREADS, "one halo dword per thread");

  __shared__ __attribute__ ((aligned (16))) uint8_t lds[2][S::NROWS * PITCH];

  /* this workgroup's tile sequence: first, first+step, ... < end (linear tile ids) */
  const uint32_t ntiles = p.map.tile_rows * p.map.tiles_x.d;
  uint32_t first, step, end;
  if (p.map.band <= 0) {
    first = blockIdx.x;
    step = gridDim.x;
    end = ntiles;
  } else {                      /* one contiguous chunk of tile rows per XCD */
    const uint32_t xcd = blockIdx.x % kNumXcd;
    const uint32_t chunk = (uint32_t) p.map.band * p.map.tiles_x.d;
    first = xcd * chunk + blockIdx.x / kNumXcd;
    step = gridDim.x / kNumXcd;
    end = (xcd + 1) * chunk < ntiles ? (xcd + 1) * chunk : ntiles;
  }
  if (first >= end)
    return;

  const int tid = threadIdx.x;
  const int c16 = (tid % S::TPR) * 16;
  const int rr = tid / S::TPR;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int wx = wave % WX;
  const int wy = wave / WX;
  const int xl = 256 * wx + 4 * lane;
  const int edge_off = (lane == 0) ? -4 : 4;
  const int r0 = wy * RPW;

  auto decode = [&](uint32_t tile) -> Tile {
    return tile_of<S::TW, S::TR> (p, linear_to_tile (tile, p.map));
  };

  u32x4 v[S::NPASS];
  uint32_t hv = 0u;
  auto issue = [&](const Tile &t) {
#pragma unroll
    for (int i = 0; i < S::NPASS; i++) {
      const int r = i * S::RPP + rr;
      const int y = t.tile_y - 1 + r;
      v[i] = (u32x4) (0u);
      if (r < S::NROWS && y <= p.height && t.tile_x + c16 < p.width)
        v[i] = *(const u32x4 *) (t.src
            + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride
            + t.tile_x + c16);
    }
    hv = 0u;
    if (tid < 2 * S::NROWS) {
      const int r = tid >> 1;
      const int y = t.tile_y - 1 + r;
      const int col = (tid & 1) ? t.tile_x + S::TW : t.tile_x - 4;
      if (y <= p.height && col >= 0 && col < p.wlimit4)
        hv = *(const uint32_t *) (t.src
            + (size_t) map_row (y, p.height, p.dn_last) * p.src_stride + col);
    }
  };
  auto commit = [&](uint8_t *buf) {
#pragma unroll
    for (int i = 0; i < S::NPASS; i++) {
      const int r = i * S::RPP + rr;
      if (r < S::NROWS)
        *(u32x4 *) &buf[r * PITCH + MAIN + c16] = v[i];
    }
    if (tid < 2 * S::NROWS)
      *(uint32_t *) &buf[(tid >> 1) * PITCH + ((tid & 1) ? MAIN + S::TW : MAIN - 4)]
          = hv;
  };
  auto compute = [&](const Tile &t, const uint8_t *buf) {
    const int x0 = t.tile_x + xl;
    const bool first_lane = (x0 == 0);
    const int lastmode = (x0 + 4 == p.width) ? 1 : 0;
    const bool active = x0 < p.width;
    const uint8_t *lrow = &buf[MAIN + xl];
    auto lines_of = [&](int r) -> Lines {
      const uint8_t *q = lrow + r * PITCH;
      const uint32_t c = *(const uint32_t *) q;
      const uint32_t edge = *(const uint32_t *) (q + edge_off);
      return row_lines<true, false> (c, from_lane_below (edge, c),
          from_lane_above (edge, c), first_lane, lastmode);
    };
    march_rows<RPW, true> (p, t.dst, t.tile_y, r0, x0, active, lines_of, [&](uint8_t *out, u32x4 px) {
      store_pixels<ST, false> (out, px, lastmode);
    });
  };

  Tile cur_tile = decode (first);
  issue (cur_tile);
  commit (lds[0]);
  __syncthreads ();
  int b = 0;
  for (uint32_t t = first; t < end; t += step) {
    const uint32_t nxt = t + step;
    const bool has_next = nxt < end;
    Tile next_tile = cur_tile;
    if (has_next) {
      next_tile = decode (nxt);
      issue (next_tile);                /* loads stay in flight across compute */
    }
    compute (cur_tile, lds[b]);
    if (has_next)
      commit (lds[b ^ 1]);
    __syncthreads ();
    b ^= 1;
    cur_tile = next_tile;
  }
}

#endif  /* MIBAYER_LAB */

/* ------------------------------------------------------------------------- */
/* variant table                                                               */
/* ------------------------------------------------------------------------- */

/* default block order per shape (measured on a dozen boxes, DESIGN.md "XCD map"):
 * 1024-px tiles -> band 1 (an XCD takes one full-width tile row at a time), the
 * only plan at 80-81.5 % of peak on EVERY box; narrower tiles -> identity */
/* tile width, tile height, threads */
#define VARIANT_SHAPE(WX, WY, RPW) 256 * (WX), (WY) * (RPW), 64 * (WX) * (WY)
#define LDS_VARIANT(name, WX, WY, RPW, NEIGH, ST, INTRIN)                      \
  { name, VARIANT_SHAPE (WX, WY, RPW), (WX) == 4 ? 1 : 0, 0,                   \
    bayer2rgb_lds_kernel<WX, WY, RPW, NEIGH, ST, INTRIN, false>,               \
    bayer2rgb_lds_kernel<WX, WY, RPW, NEIGH, ST, INTRIN, true>, nullptr, nullptr }
/* production shapes and their plain-store twins: + the sector-aligned arms for generic geometries (the 64-byte
 * flavour only in the lab build: the autotuner's candidates use the 128-byte one) */
#ifdef MIBAYER_LAB
#define ALIGNED64_ARM(WX, WY, RPW, ST) bayer2rgb_lds_aligned_kernel<WX, WY, RPW, ST, 64>
#else
#define ALIGNED64_ARM(WX, WY, RPW, ST) nullptr
#endif
#define LDS_VARIANT_AL(name, WX, WY, RPW, ST)                                  \
  { name, VARIANT_SHAPE (WX, WY, RPW), (WX) == 4 ? 1 : 0, 0,                   \
    bayer2rgb_lds_kernel<WX, WY, RPW, 0, ST, true, false>,                     \
    bayer2rgb_lds_kernel<WX, WY, RPW, 0, ST, true, true>,                      \
    ALIGNED64_ARM (WX, WY, RPW, ST),                                           \
    bayer2rgb_lds_aligned_kernel<WX, WY, RPW, ST, 128> }
#ifdef MIBAYER_LAB
#define PERSIST_VARIANT(name, WX, WY, RPW, ST)                                 \
  { name, VARIANT_SHAPE (WX, WY, RPW), -1, 1,                                  \
    bayer2rgb_persist_kernel<WX, WY, RPW, ST>,                                 \
    bayer2rgb_lds_kernel<WX, WY, RPW, 0, ST, true, true>, nullptr, nullptr }
#define DIRECT_VARIANT(name, WX, WY, RPW, ST, INTRIN)                          \
  { name, VARIANT_SHAPE (WX, WY, RPW), -1, 0,                                  \
    bayer2rgb_direct_kernel<WX, WY, RPW, ST, INTRIN, false>,                   \
    bayer2rgb_direct_kernel<WX, WY, RPW, ST, INTRIN, true>, nullptr, nullptr }
#endif

/* Measured on MI355X (profiles/sweep_r01_*.log, interleaved A/B, 4K x 64 frames):
 * 4 rows per wave and 8 waves per workgroup is the sweet spot (83-84 % of the
 * 8 TB/s HBM peak); 8 rows per wave costs 3 points, 2 rows per wave 15; nt
 * stores gain 1.3 points over plain stores, sc1 / sc0 sc1 stores lose 2; DPP,
 * ds_bpermute and LDS neighbour reads tie; the no-LDS arm loses 15 points. */
static const Variant kVariants[] = {
  /* 0: "auto" -- resolved per stream width by resolve_variant() below */
  { "auto", 0, 0, 0, -1, 0, nullptr, nullptr, nullptr, nullptr },
  /* 1-3: the production shapes (tile 1024x8, 512x16, 256x32; 512 threads), streaming (nt) stores */
  LDS_VARIANT_AL ("lds_4x2_r4_dpp_nt", 4, 2, 4, 1),
  LDS_VARIANT_AL ("lds_2x4_r4_dpp_nt", 2, 4, 4, 1),
  LDS_VARIANT_AL ("lds_1x8_r4_dpp_nt", 1, 8, 4, 1),
  /* 4-6: the same shapes with plain (write-back) stores: for output rows that start off a 64-byte sector
   * (width % 16 != 0) the L2 then completes the partial sectors two waves share before they go out */
  LDS_VARIANT_AL ("lds_4x2_r4_dpp", 4, 2, 4, 0),
  LDS_VARIANT_AL ("lds_2x4_r4_dpp", 2, 4, 4, 0),
  LDS_VARIANT_AL ("lds_1x8_r4_dpp", 1, 8, 4, 0),
  /* 7-9: the hybrid store policy (generic geometries: nt for the lines a wave-store covers completely, write-back for
   * its ragged ends; sector-aligned geometries: nt) */
  LDS_VARIANT ("lds_4x2_r4_dpp_hy", 4, 2, 4, 0, 5, true),
  LDS_VARIANT ("lds_2x4_r4_dpp_hy", 2, 4, 4, 0, 5, true),
  LDS_VARIANT ("lds_1x8_r4_dpp_hy", 1, 8, 4, 0, 5, true),
#ifdef MIBAYER_LAB
  /* 10.. : tuning / verification arms of the lab build (`make lab`), all bit-exact (tests/test_gpu_lab_arms.py);
   * what each of them measured is in profiles/r01_sweep_*.log */
  LDS_VARIANT ("lds_1x8_r4_dpp_sc1", 1, 8, 4, 0, 2, true),
  LDS_VARIANT ("lds_1x8_r4_shfl_nt", 1, 8, 4, 1, 1, true),
  LDS_VARIANT ("lds_1x8_r4_ldsnb_nt", 1, 8, 4, 2, 1, true),
  LDS_VARIANT ("lds_1x8_r4_ldsnb_swar", 1, 8, 4, 2, 0, false),
  LDS_VARIANT ("lds_1x4_r8_dpp_nt", 1, 4, 8, 0, 1, true),
  LDS_VARIANT ("lds_1x16_r4_dpp_nt", 1, 16, 4, 0, 1, true),
  LDS_VARIANT ("lds_1x8_r2_dpp_nt", 1, 8, 2, 0, 1, true),
  LDS_VARIANT ("lds_4x1_r16_dpp_nt", 4, 1, 16, 0, 1, true),
  DIRECT_VARIANT ("direct_1x4_r8_nt", 1, 4, 8, 1, true),
  LDS_VARIANT ("lds_1x1_r4_dpp_nt", 1, 1, 4, 0, 1, true),
  LDS_VARIANT ("lds_1x4_r4_dpp_nt", 1, 4, 4, 0, 1, true),
  /* negative result kept as a verified arm: 64-68 % of peak vs 77-80 % for the
   * per-tile kernels in the same interleaved run (profiles/r01_sweep_persistent.log) */
  PERSIST_VARIANT ("persist_4x2_r4_nt", 4, 2, 4, 1),
  PERSIST_VARIANT ("persist_1x8_r4_nt", 1, 8, 4, 1),
  /* nt hint on the row loads as well (the mosaic is read once per XCD) */
  LDS_VARIANT ("lds_4x2_r4_dpp_nt_ldnt", 4, 2, 4, 0, 9, true),
  /* direct global -> LDS row loads (no staging registers, no ds_write pass) */
  LDS_VARIANT ("lds_4x2_r4_dpp_nt_glds", 4, 2, 4, 0, 17, true),
#endif
};

int variant_count ()
{
  return (int) (sizeof (kVariants) / sizeof (kVariants[0]));
}

const Variant &variant (int id)
{
  return kVariants[id];
}

/* Output rows that do not start on a 64-byte sector (4 * width, or a padded stride, not a multiple of
 * 64: 4056-px sensors, any width % 16 != 0): every wave-store of a row then ends in a partial sector that the
 * neighbouring wave -- or the neighbouring workgroup -- completes.  Streaming (nt) stores push those halves out
 * one by one; plain write-back stores let the L2 put them together first, provided both halves reach the SAME
 * L2, i.e. under the chunk-per-XCD order: 4056x3040 76.0 -> 78.9 %, 3838x2160 72.5 -> 78.5 %, 1366x768
 * 68.1 -> 73.3 % of peak (profiles/r02_generic_path.log); for sector-aligned rows nt + band 1 stays ahead
 * (80.8 vs 79.3 %).  Ids: production shape s in 1..3 -> plain-store twin s + 3, hybrid-store twin s + 6. */
int plain_store_twin (int id)
{
  return (id >= 1 && id <= 3) ? id + 3 : id;
}

/* the hybrid-store arm of a production shape (store_pixels_hybrid: nt inside, write-back at the ragged ends of a
 * wave-store), for generic geometries whose output rows are 16-byte aligned but off the line grid */
int hybrid_store_twin (int id)
{
  return (id >= 1 && id <= 3) ? id + 6 : id;
}

/* the production shape (ids 1-3) a plain-store or hybrid-store twin stands for; any other id is returned unchanged */
int production_shape_of (int id)
{
  return (id >= 4 && id <= 9) ? (id - 1) % 3 + 1 : id;
}

/* variant 0.  Rows that fit into ONE tile take the narrowest production tile that covers them (256 / 512 / 1024 px),
 * run in identity order without the start delay: 81-84 % of HBM peak for 320 ... 1024-px rows, against 50-79 % for
 * the other shapes (a second, mostly empty tile per row is what hurts: 640 px in 512-px tiles 59 %;
 * profiles/r01_sweep_narrow_frames.log).  Wider rows: 1024x8 tiles whenever they pad the frame width by no more
 * than 7 % beyond the best shape (3840 -> 4096 is fine) -- with the band-1 order they are the robust plan --
 * otherwise the production shape that wastes the fewest lanes, the widest among equals. */
int resolve_variant (int id, int width)
{
  if (id != 0)
    return id;
  if (width <= 256)
    return 3;
  if (width <= 512)
    return 2;
  if (width <= 1024)
    return 1;
  static const int tile_w[3] = { 1024, 512, 256 };      /* variants 1, 2, 3 */
  long long padded[3];
  int best = 0;
  for (int i = 0; i < 3; i++) {
    padded[i] = (long long) ((width + tile_w[i] - 1) / tile_w[i]) * tile_w[i];
    if (padded[i] < padded[best])
      best = i;
  }
  if (padded[0] * 100 <= padded[best] * 107)
    return 1;
  return best + 1;
}

/* Batch-class default for widths whose measured winner the rules above do not find.  Every entry beat the rule's pick
 * by the margin noted, on two boxes in two rounds (profiles/r04_plan_sweep_530Mpix.log, r05_plan_sweep_530Mpix.log:
 * ~530-Mpixel batches, 3 shapes x {band 1, identity}; the chunk order is left out on purpose -- whether it is fast
 * follows the allocation, DESIGN.md section 5 -- and stays the measured plan's business).  The rules cannot see these:
 * which block order collides in the memory channels depends on the row pitch in ways the sweeps show (3264 px in
 * 1024x8 tiles, identity order: 69 %; 2592 px in 512x16: 71 %) but nothing here models.  Sector-aligned geometries
 * with cfg.variant == 0 only; anything measured (mibayer_autotune, the plan cache) still overrides it. */
bool known_width_plan (int width, int *variant, int *band)
{
  static const struct { int width, variant, band; } kKnown[] = {
    { 2048, 3, 1 },     /* 256x32 band 1: 83.3 / 84.1 % against 82.3 / 82.6 (1024x8 identity) */
    { 4096, 3, 1 },     /*                83.3 / 83.7          81.0 / 81.2                     */
    { 8192, 3, 1 },     /*                81.9 / 82.7          81.1 / 82.0                     */
    { 2304, 2, 0 },     /* 512x16 identity: 80.7 / 80.6 against 78.8 / 78.8 (256x32 identity)  */
    { 3264, 2, 0 },     /*                  80.1 / 79.2          78.4 / 77.9                   */
    { 2448, 1, 0 },     /* 1024x8 identity: 79.5 / 79.8 against 77.7 / 78.3 (512x16 identity); 2448x2048: 79.1 / 76.8 */
    { 2560, 1, 0 },     /*                  81.1 / 81.2          79.2 / 78.9                   */
    { 2592, 1, 0 },     /*                  81.3 / 81.7          79.3 / 79.6 (256x32 identity) */
    { 2688, 1, 0 },     /*                  82.4 / 82.4          77.4 / 77.5 (256x32 identity) */
    { 4608, 1, 0 },     /*                  82.4 / 81.2          79.5 / 79.4 (512x16 identity) */
    { 4112, 2, 1 },     /* 512x16 band 1:   79.6 / 79.9 against 77.8 / 77.0 (256x32 identity)  */
    { 4208, 2, 1 },     /*                  78.9 / 79.8          77.1 / 77.3                   */
    { 6000, 2, 1 },     /*                  78.0 / 77.9          76.8 / 75.4 (1024x8 band 1)   */
  };
  for (const auto &k : kKnown)
    if (k.width == width) {
      *variant = k.variant;
      *band = k.band;
      return true;
    }
  return false;
}

/* Variant 0 for a launch of ONE frame (PLAN_FRAME, mibayer_abi.hip): such a launch is a handful of rounds of
 * workgroups at most -- a 4K frame in 1024x8 tiles is 1080 workgroups on the 1024 slots of 256 CUs x 4, i.e. a second
 * round that is 5 % full -- so the shape whose grid needs the fewest rounds wins (4K: 256x32 tiles = 1020 workgroups,
 * one round: 54.8 vs 47.9 % of peak launched frame by frame; 3264x2448: 53.9 vs 49.9 %; 8K: 512x16 = 3.96 rounds
 * against 4.25: 68.0 vs 64.2 %), the widest tile among equals (2592x1944, all one round: 47.1 / 45.7 / 44.6 %;
 * 4056x3040, all two: 53.6 / 51.8 / 47.7 %) -- profiles/r05_single_frame.md.  Rows that fit one tile keep the rule of
 * resolve_variant().  `slots`: workgroups resident at once (CUs x 4 for the 512-thread production shapes). */
int frame_class_variant (int width, int height, int slots)
{
  if (width <= 1024 || slots < 1)
    return resolve_variant (0, width);
  static const int tile_w[3] = { 1024, 512, 256 }, tile_h[3] = { 8, 16, 32 };      /* variants 1, 2, 3 */
  int best = 0;
  long long best_rounds = 0;
  for (int i = 0; i < 3; i++) {
    const long long tiles = (long long) ((width + tile_w[i] - 1) / tile_w[i]) * ((height + tile_h[i] - 1) / tile_h[i]);
    const long long rounds = (tiles + slots - 1) / slots;
    if (i == 0 || rounds < best_rounds) {
      best = i;
      best_rounds = rounds;
    }
  }
  return best + 1;
}

/* ------------------------------------------------------------------------- */
/* rgb2bayer: the sibling element's per-pixel gather                           */
/* ------------------------------------------------------------------------- */
/* Reference gst/bayer/gstrgb2bayer.c:254-268: output byte (j,i) is one channel
 * of input pixel (j,i), chosen by the CFA site ((j&1)<<1)|(i&1).  4 B read +
 * 1 B written per pixel: a read-dominated HBM stream.  A lane converts 4 pixels
 * (16 B in, one dword out); a 256-thread block walks R2B_ROWS rows of a
 * 1024-pixel column strip so every lane keeps several 16-byte loads in flight.
 * The two v_perm_b32 selectors per row parity come from the host. */
template <bool VEC16, int R2B_ROWS>
__global__ void __launch_bounds__ (256)
rgb2bayer_kernel (R2BParams p)
{
  /* same XCD-aware block -> tile map as the demosaic kernel: a "tile" is
   * R2B_ROWS rows x 1024 pixels, tile rows run through the whole batch */
  const TileId tile = block_to_tile (blockIdx.x, p.map);
  if (!tile.valid)
    return;
  const int xd = (int) tile.tx * 256 + threadIdx.x;     /* output dword in the row */
  if (xd >= p.out_dwords)
    return;
  for (int z = 0; z < p.start_sleep; z++)
    __builtin_amdgcn_s_sleep (1);
  const long long row0 = (long long) tile.row * R2B_ROWS;
  const int x0 = xd * 4;
  /* (frame, y) of row0; later rows only increment */
  const uint32_t f0 = fastdiv ((uint32_t) row0, p.div_height);
  const int y0 = (int) ((uint32_t) row0 - f0 * p.div_height.d);
  u32x4 px[R2B_ROWS];
#pragma unroll
  for (int k = 0; k < R2B_ROWS; k++) {
    const long long row = row0 + k;
    px[k] = (u32x4) (0u);
    if (row < p.total_rows) {
      int y = y0 + k;
      uint32_t f = f0;
      while (y >= p.height) {
        y -= p.height;
        f++;
      }
      const uint8_t *s = p.src + f * p.src_frame_bytes
          + (size_t) y * p.src_stride + (size_t) x0 * 4;
      if constexpr (VEC16) {
        px[k] = *(const u32x4 *) s;
      } else {
        const uint32_t *q = (const uint32_t *) s;
        if (x0 + 0 < p.width) px[k].x = q[0];
        if (x0 + 1 < p.width) px[k].y = q[1];
        if (x0 + 2 < p.width) px[k].z = q[2];
        if (x0 + 3 < p.width) px[k].w = q[3];
      }
    }
  }
  /* columns >= width inside the last dword are written as 0 */
  const int valid = p.width - x0;
  const uint32_t keep = valid >= 4 ? 0xffffffffu : ((1u << (8 * valid)) - 1u);
#pragma unroll
  for (int k = 0; k < R2B_ROWS; k++) {
    const long long row = row0 + k;
    if (row < p.total_rows) {
      int y = y0 + k;
      uint32_t f = f0;
      while (y >= p.height) {
        y -= p.height;
        f++;
      }
      const int par = y & 1;
      const uint32_t lo = __builtin_amdgcn_perm (px[k].y, px[k].x, p.sel_lo[par]);
      const uint32_t hi = __builtin_amdgcn_perm (px[k].w, px[k].z, p.sel_hi[par]);
      uint32_t *d = (uint32_t *) (p.dst + f * p.dst_frame_bytes
          + (size_t) y * p.dst_stride + (size_t) x0);
      __builtin_nontemporal_store ((lo | hi) & keep, d);
    }
  }
}

/* Flat form: with no neighbourhood the batch is one linear sequence of 4-pixel
 * items (16 B in -> one dword out); only the row parity (which pair of v_perm
 * selectors) and, for padded strides, the addresses depend on where an item sits.
 * No lane is wasted on a partial last tile (3840 px = 3.75 tiles of 1024 in the
 * tile kernel: 6 % idle lanes), every thread keeps K groups of loads in flight,
 * and with PX == 8 a lane owns 32 contiguous input bytes and stores 8 bytes
 * (512 B per wave-store instead of 256).  Items are decoded with two
 * multiply-shift divisions (row = item / dwords-per-row, frame = row / height). */
/* VEC = 16: width % 4 == 0 and 16-byte aligned frames -- every item is full and loaded
 * unconditionally.  VEC = 4: any other geometry -- full items still take one 16-byte load (at
 * dword alignment, which is all a gfx950 global load needs), the partial last item of a row is
 * read dword by dword */
/* The frame index is block-uniform and the table sits in the kernel arguments: read it straight out of the kernarg
 * segment (a scalar load at a run-time offset).  Indexing the by-value copy `p` instead made the compiler keep the
 * whole 480-byte argument block in scratch memory in this kernel (488 bytes per lane, 20x slower): R2BParams is the
 * kernel's only argument, so it starts at offset 0 of the segment. */
template <typename T>
__device__ __forceinline__ T kernarg_table_entry (size_t table_offset, uint32_t index)
{
  typedef const __attribute__ ((address_space (4))) char *kptr;
  kptr base = (kptr) __builtin_amdgcn_kernarg_segment_ptr ();
  return ((const __attribute__ ((address_space (4))) T *) (base + table_offset))[index];
}

template <int K, int PX, int LD, int VEC>
__global__ void __launch_bounds__ (256)
rgb2bayer_flat_kernel (R2BParams p)
{
  constexpr bool VEC16 = VEC == 16;
  constexpr int IPG = PX / 4;           /* items per group */
  const TileId tile = block_to_tile (blockIdx.x, p.map);       /* tiles_x == 1: .row = logical block */
  if (!tile.valid)
    return;
  for (int z = 0; z < p.start_sleep; z++)
    __builtin_amdgcn_s_sleep (1);
  /* list launch: this block's frame (block-uniform) and its first item inside that frame */
  const uint32_t lframe = p.nlist ? fastdiv (tile.row, p.div_blocks_per_frame) : 0u;
  const uint32_t lblock = tile.row - lframe * p.div_blocks_per_frame.d;
  const uint8_t *src_base = p.nlist
      ? kernarg_table_entry<const uint8_t *> (offsetof (R2BParams, src_list), lframe) : p.src;
  uint8_t *dst_base = p.nlist
      ? kernarg_table_entry<uint8_t *> (offsetof (R2BParams, dst_list), lframe) : p.dst;
  const uint32_t first = p.item0 + (lblock * (uint32_t) (256 * K) + threadIdx.x) * IPG;
  u32x4 px[K][IPG];
  uint32_t par[K];
  size_t doff[K];               /* byte offset into dst_base (kept as an offset: the stores stay global_store) */
  bool valid[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const uint32_t item = first + (uint32_t) k * 256u * IPG;
#pragma unroll
    for (int h = 0; h < IPG; h++)
      px[k][h] = (u32x4) (0u);
    par[k] = 0;
    doff[k] = 0;
    valid[k] = item < p.item_end;
    if (valid[k]) {
      const uint32_t row = fastdiv (item, p.div_out_dwords);
      const uint32_t xd = item - row * p.div_out_dwords.d;
      /* list launch: items count inside the block's own frame, so row == y */
      const uint32_t f = p.nlist ? 0u : fastdiv (row, p.div_height);
      const uint32_t y = row - f * p.div_height.d;
      par[k] = y & 1u;
      const uint8_t *s = src_base + f * p.src_frame_bytes + (size_t) y * p.src_stride
          + (size_t) xd * 16;
      doff[k] = f * p.dst_frame_bytes + (size_t) y * p.dst_stride + (size_t) xd * 4;
#pragma unroll
      for (int h = 0; h < IPG; h++) {
        if constexpr (VEC16) {
          if constexpr (LD == 1)
            px[k][h] = __builtin_nontemporal_load ((const u32x4 *) s + h);
          else
            px[k][h] = ((const u32x4 *) s)[h];
        } else {
          const uint32_t *q = (const uint32_t *) s + 4 * h;
          const int x0 = (int) (xd + h) * 4;
          if (x0 + 3 < p.width) {
            /* a full item: one 16-byte load at the alignment the rows have (gfx950 global
             * loads need no more than dword alignment) */
            typedef uint32_t u32x4_a4 __attribute__ ((ext_vector_type (4), aligned (4)));
            if constexpr (LD == 1)
              px[k][h] = __builtin_nontemporal_load ((const u32x4_a4 *) q);
            else
              px[k][h] = *(const u32x4_a4 *) q;
          } else {
            if (x0 + 0 < p.width) px[k][h].x = q[0];
            if (x0 + 1 < p.width) px[k][h].y = q[1];
            if (x0 + 2 < p.width) px[k][h].z = q[2];
            if (x0 + 3 < p.width) px[k][h].w = q[3];
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    if (valid[k]) {
      /* both selector pairs live in SGPRs: a select, not an indexed kernarg load */
      const uint32_t sel_lo = par[k] ? p.sel_lo[1] : p.sel_lo[0];
      const uint32_t sel_hi = par[k] ? p.sel_hi[1] : p.sel_hi[0];
      uint32_t out[IPG];
#pragma unroll
      for (int h = 0; h < IPG; h++) {
        /* pixels that were not loaded (x >= width) are zero, and so are their output bytes */
        const uint32_t lo = __builtin_amdgcn_perm (px[k][h].y, px[k][h].x, sel_lo);
        const uint32_t hi = __builtin_amdgcn_perm (px[k][h].w, px[k][h].z, sel_hi);
        out[h] = lo | hi;
      }
      uint8_t *d = dst_base + doff[k];
      if constexpr (IPG == 2) {
        u32x2 v;
        v.x = out[0];
        v.y = out[1];
        __builtin_nontemporal_store (v, (u32x2 *) d);
      } else {
        __builtin_nontemporal_store (out[0], (uint32_t *) d);
      }
    }
  }
}

typedef void (*R2BFn) (R2BParams);

template <int VEC>
static R2BFn flat_kernel_for (int k, int px, int ld)
{
#define R2B_FLAT(K, PX, LD) if (k == K && px == PX && ld == LD) return rgb2bayer_flat_kernel<K, PX, LD, VEC>
#ifndef MIBAYER_LAB
  R2B_FLAT (2, 4, 1);           /* the production launch shape (profiles/r02_rgb2bayer_sweep.log) */
#else
  R2B_FLAT (1, 4, 0); R2B_FLAT (1, 4, 1); R2B_FLAT (1, 8, 0); R2B_FLAT (1, 8, 1);
  R2B_FLAT (2, 4, 0); R2B_FLAT (2, 4, 1); R2B_FLAT (2, 8, 0); R2B_FLAT (2, 8, 1);
  R2B_FLAT (3, 4, 0); R2B_FLAT (3, 4, 1); R2B_FLAT (3, 8, 0); R2B_FLAT (3, 8, 1);
  R2B_FLAT (4, 4, 0); R2B_FLAT (4, 4, 1); R2B_FLAT (4, 8, 0); R2B_FLAT (4, 8, 1);
  R2B_FLAT (8, 4, 0); R2B_FLAT (8, 4, 1); R2B_FLAT (8, 8, 0); R2B_FLAT (8, 8, 1);
#endif
#undef R2B_FLAT
  return nullptr;
}

static bool aligned_to (const void *ptr, unsigned a)
{
  return (((uintptr_t) ptr) & (a - 1)) == 0;
}

/* The flat-kernel launch of items [q.item0, q.item_end): of the batch as one sequence, or (q.nlist) of each frame of
 * the list, every frame a whole number of blocks.  dst8: every destination 8-byte aligned (two items per store
 * allowed).  false: this build has no flat kernel of that shape and nothing was launched */
static bool launch_flat (R2BParams &q, bool vec16, bool dst8, hipStream_t stream, hipError_t *err)
{
  int px = q.flat_px == 8 ? 8 : 4;
  /* two items per group: they must be in one row and the 8-byte store aligned */
  if (px == 8 && ((q.out_dwords & 1) || (q.dst_stride & 7) || !dst8 || !vec16))
    px = 4;
  R2BFn fn = vec16 ? flat_kernel_for<16> (q.flat_k, px, q.flat_ld ? 1 : 0)
      : flat_kernel_for<4> (q.flat_k, px, q.flat_ld ? 1 : 0);
  if (!fn)
    return false;
  const long long items = (long long) q.item_end - q.item0;
  const long long per_block = 256LL * q.flat_k * (px / 4);
  long long nblocks = (items + per_block - 1) / per_block;
  if (q.nlist) {
    q.div_blocks_per_frame = make_fastdiv ((uint32_t) nblocks);
    nblocks *= q.nlist;
  }
  if (q.band < 0)               /* one contiguous chunk of the launch per XCD */
    q.band = (int) ((nblocks + kNumXcd - 1) / kNumXcd);
  const long long grid = grid_blocks_for (1, nblocks, q.band);
  *err = hipErrorInvalidValue;
  if (grid <= 0x7fffffffLL) {
    q.map = make_tile_map (1, 1, nblocks, q.band, 0);
    hipLaunchKernelGGL (fn, dim3 ((unsigned) grid), dim3 (256), 0, stream, q);
    *err = hipGetLastError ();
  }
  return true;
}

hipError_t launch_rgb2bayer (const R2BParams &p, bool vec16, hipStream_t stream,
    long long row0, long long nrows)
{
  if (p.total_rows <= 0 || p.out_dwords <= 0 || nrows == 0)
    return hipSuccess;
  R2BParams q = p;
  if (nrows < 0) {
    row0 = 0;
    nrows = p.total_rows;
  }
  if (row0 < 0 || (row0 & 15) || row0 + nrows > p.total_rows)
    return hipErrorInvalidValue;
  if (p.total_rows > 0x7fffffffLL)
    return hipErrorInvalidValue;
  q.div_height = make_fastdiv ((uint32_t) p.height);
  q.div_out_dwords = make_fastdiv ((uint32_t) p.out_dwords);

  /* ---- flat kernel ---------------------------------------------------------- */
  const long long item_end = (row0 + nrows) * p.out_dwords;
  if (q.flat_k > 0 && item_end <= 0x7fffffffLL) {
    q.item0 = (uint32_t) (row0 * p.out_dwords);
    q.item_end = (uint32_t) item_end;
    hipError_t err;
    if (launch_flat (q, vec16, !(p.dst_frame_bytes & 7) && aligned_to (p.dst, 8), stream, &err))
      return err;
  }

  /* ---- tile kernel ------------------------------------------------------------ */
  q.total_rows = row0 + nrows;  /* the kernel's "row < total_rows" guard ends the band */
#ifdef MIBAYER_LAB
  const int R2B_ROWS = (q.rows == 4 || q.rows == 8 || q.rows == 16) ? q.rows : 2;
#else
  const int R2B_ROWS = 2;       /* the product build carries the tile kernel as the fallback for batches too long for
                                   the flat kernel's 32-bit item index, in one shape */
#endif
  const long long tile_rows = (nrows + R2B_ROWS - 1) / R2B_ROWS;
  const int tiles_x = (p.out_dwords + 255) / 256;
  if (q.band < 0)               /* one contiguous chunk of tile rows per XCD */
    q.band = (int) ((tile_rows + kNumXcd - 1) / kNumXcd);
  const long long grid = grid_blocks_for (tiles_x, tile_rows, q.band);
  if (grid > 0x7fffffffLL)
    return hipErrorInvalidValue;
  q.map = make_tile_map (tiles_x, 1, tile_rows, q.band, row0 / R2B_ROWS);
#define R2B_LAUNCH(V, R) hipLaunchKernelGGL ((rgb2bayer_kernel<V, R>), \
      dim3 ((unsigned) grid), dim3 (256), 0, stream, q)
  switch (R2B_ROWS * 2 + (vec16 ? 1 : 0)) {
    case 2 * 2 + 1: R2B_LAUNCH (true, 2); break;
#ifndef MIBAYER_LAB
    default: R2B_LAUNCH (false, 2); break;
#else
    case 2 * 2 + 0: R2B_LAUNCH (false, 2); break;
    case 4 * 2 + 1: R2B_LAUNCH (true, 4); break;
    case 4 * 2 + 0: R2B_LAUNCH (false, 4); break;
    case 8 * 2 + 1: R2B_LAUNCH (true, 8); break;
    case 8 * 2 + 0: R2B_LAUNCH (false, 8); break;
    case 16 * 2 + 1: R2B_LAUNCH (true, 16); break;
    default: R2B_LAUNCH (false, 16); break;
#endif
  }
#undef R2B_LAUNCH
  return hipGetLastError ();
}

/* reference loop per frame: gst/bayer/gstrgb2bayer.c:254-268; here up to kMaxList frames, each its own allocation,
 * in one launch of the flat kernel */
hipError_t launch_rgb2bayer_list (const R2BParams &p, bool vec16, bool dst8, hipStream_t stream)
{
  if (p.nlist <= 0 || p.height <= 0 || p.out_dwords <= 0)
    return hipSuccess;
  if (p.nlist > kMaxList || p.flat_k <= 0)
    return hipErrorInvalidValue;
  R2BParams q = p;
  q.total_rows = p.height;
  q.div_height = make_fastdiv ((uint32_t) p.height);
  q.div_out_dwords = make_fastdiv ((uint32_t) p.out_dwords);
  const long long items = (long long) p.height * p.out_dwords;
  if (items > 0x7fffffffLL)
    return hipErrorInvalidValue;
  q.item0 = 0;
  q.item_end = (uint32_t) items;
  hipError_t err;
  return launch_flat (q, vec16, dst8, stream, &err) ? err : hipErrorInvalidValue;
}

/* ------------------------------------------------------------------------- */
/* deep samples: 10-16-bit mosaics in 16-bit words, 16-bit-per-channel output  */
/* ------------------------------------------------------------------------- */
/* The closed form of the file header on samples of `bits` significant bits (the word masked to them), every average
 * at the native depth, the conversion to the output depth last: 16-bit channels v << (16 - bits) (alpha 0xffff),
 * 8-bit channels v >> (bits - 8) (alpha 255).  An 8-bit mosaic with 16-bit output is bits = 8.
 *
 * A lane owns 4 horizontally adjacent pixels as two dwords of two 16-bit samples each (lo = pixels 0,1, hi = 2,3), a
 * wave a strip of 256 pixels x kStripRows rows: it loads all kStripRows + 2 source rows first (the loads of a lane are all
 * in flight at once), then walks down with the 3-row window (E,O of rows u, j, d) in registers.  Two samples per dword: avg is exact per half without packed
 * instructions ((a|b) - (((a^b) >> 1) & 0x7fff7fff): no borrow crosses the halves), the output shift cannot cross
 * them either.  The x-1 / x+4 neighbours come from the adjacent lanes by DPP; lanes 0 and 63 load theirs.  Output
 * pixels are v_perm_b32 of {R'B' word, G word} with selectors from the host (layout, Bayer order, output byte order):
 * 16-bit output 32 bytes per lane (two global_store_dwordx4, pieces swapped inside a quad), 8-bit output 16 bytes
 * (one, streaming).  Rows need only be
 * dword-aligned (gfx950 vector memory at dword alignment); the partial last group of a width % 4 == 2 row loads one
 * dword and stores two pixels. */

constexpr uint32_t kLowHalves = 0x0000ffffu;

__device__ __forceinline__ uint32_t avg16x2 (uint32_t a, uint32_t b)
{
  return (a | b) - (((a ^ b) >> 1) & 0x7fff7fffu);
}

/* the source dwords of one row as loaded: a = pixels 0,1 (8-bit mosaic: pixels 0..3), b = pixels 2,3, e = the edge
 * dword -- the two samples left of the strip in lane 0, right of it in lane 63.  They are converted (byte order, mask,
 * 8-bit unpack) only where they are used, so that no load waits for another. */
struct DeepRaw { uint32_t a, b, e; };
struct DeepLines { uint32_t elo, ehi, olo, ohi; };

/* loads row y of the frame at `base`: lane group g (x0 = 4g) */
template <bool IN8>
__device__ __forceinline__ DeepRaw deep_load (const DeepParams &p, const uint8_t *base, int y, int g, int lane)
{
  DeepRaw r = { 0u, 0u, 0u };
  const uint8_t *row = base + (size_t) y * (size_t) p.src_stride;
  const int x0 = 4 * g;
  /* one load instruction per register and no branch between a load and its use: a load into a register that another
   * load of the same row may still be filling would wait for it */
  if (g < p.groups) {
    if constexpr (IN8) {
      r.a = __builtin_nontemporal_load ((const uint32_t *) (row + x0));
    } else {
      /* width % 4 == 2, last group: pixels x0, x0+1 only -- the 8 bytes that end with them (x0 >= 4 there);
       * deep_lines picks them out of b */
      const u32x2_a4 c = __builtin_nontemporal_load ((const u32x2_a4 *) (row + 2 * x0 - (x0 + 4 <= p.width ? 0 : 4)));
      r.a = c.x;
      r.b = c.y;
    }
  }
  const bool left = lane == 0 && x0 > 0 && g < p.groups;        /* samples x0-2, x0-1 */
  const bool right = lane == 63 && x0 + 4 < p.width;            /* samples x0+4, x0+5 */
  if (left || right)
    r.e = *(const uint32_t *) (row + (IN8 ? (left ? x0 - 4 : x0 + 4) : 2 * (left ? x0 - 2 : x0 + 4)));
  return r;
}

/* E / O of one row (reference gstbayer2rgb.c:354-381) with the edge columns O[0] = S[1], E[W-1] = S[W-2],
 * O[W-2] = S[W-3]: first = group 0; lastmode 1 = last group of a width % 4 == 0 row, 2 = of a width % 4 == 2 row.
 * The samples are masked, in host byte order, two per dword. */
template <bool IN8>
__device__ __forceinline__ DeepLines deep_lines (const DeepParams &p, const DeepRaw &raw, int lane, bool first,
    int lastmode)
{
  const bool partial = lastmode == 2;
  uint32_t lo, hi, e;
  if constexpr (IN8) {
    lo = __builtin_amdgcn_perm (raw.a, raw.a, 0x0c010c00u);
    hi = __builtin_amdgcn_perm (raw.a, raw.a, 0x0c030c02u);
    e = __builtin_amdgcn_perm (raw.e, raw.e, lane == 0 ? 0x0c030c02u : 0x0c010c00u);
  } else {
    const uint32_t a = partial ? raw.b : raw.a;
    lo = __builtin_amdgcn_perm (a, a, p.in_sel) & p.mask2;
    hi = partial ? 0u : __builtin_amdgcn_perm (raw.b, raw.b, p.in_sel) & p.mask2;
    e = __builtin_amdgcn_perm (raw.e, raw.e, p.in_sel) & p.mask2;
  }
  const uint32_t left_hi = from_lane_below (e, hi);             /* [S x0-2, S x0-1] */
  const uint32_t right_lo = from_lane_above (e, lo);            /* [S x0+4, S x0+5] */
  const uint32_t mid = __builtin_amdgcn_alignbit (hi, lo, 16);                  /* [s1, s2] */
  const uint32_t lsh = first ? __builtin_amdgcn_alignbit (lo, lo, 16)           /* [s1, s0] */
      : __builtin_amdgcn_alignbit (lo, left_hi, 16);                            /* [S x0-1, s0] */
  const uint32_t rsh = __builtin_amdgcn_alignbit (right_lo, hi, 16);           /* [s3, S x0+4] */
  const uint32_t a_lo = avg16x2 (lsh, lastmode == 2 ? lsh : mid);
  const uint32_t a_hi = avg16x2 (mid, lastmode == 1 ? mid : rsh);
  DeepLines l;
  l.elo = bsel (kLowHalves, lo, a_lo);
  l.ehi = bsel (kLowHalves, hi, a_hi);
  l.olo = bsel (kLowHalves, a_lo, lo);
  l.ohi = bsel (kLowHalves, a_hi, hi);
  return l;
}

/* lane k of a quad: s0 = piece k of the quad's first 64 output bytes (lane k>>1, its v0 / v1 for k even / odd),
 * s1 = piece k of its last 64 (lane 2 + (k>>1)) */
template <int CTRL>
__device__ __forceinline__ u32x4 quad_dpp (u32x4 v)
{
  u32x4 r;
  r.x = (uint32_t) __builtin_amdgcn_mov_dpp ((int) v.x, CTRL, 0xf, 0xf, false);
  r.y = (uint32_t) __builtin_amdgcn_mov_dpp ((int) v.y, CTRL, 0xf, 0xf, false);
  r.z = (uint32_t) __builtin_amdgcn_mov_dpp ((int) v.z, CTRL, 0xf, 0xf, false);
  r.w = (uint32_t) __builtin_amdgcn_mov_dpp ((int) v.w, CTRL, 0xf, 0xf, false);
  return r;
}

__device__ __forceinline__ void deep_quad_pieces (u32x4 v0, u32x4 v1, int k, u32x4 &s0, u32x4 &s1)
{
  constexpr int kLow = 0x50;            /* quad_perm [0,0,1,1]: lane k reads lane k>>1 */
  constexpr int kHigh = 0xfa;           /* quad_perm [2,2,3,3]: lane k reads lane 2 + (k>>1) */
  /* every lane runs all four moves (a DPP source lane must be active), then picks */
  const u32x4 l0 = quad_dpp<kLow> (v0), l1 = quad_dpp<kLow> (v1);
  const u32x4 h0 = quad_dpp<kHigh> (v0), h1 = quad_dpp<kHigh> (v1);
  s0 = (k & 1) ? l1 : l0;
  s1 = (k & 1) ? h1 : h0;
}

/* 4-byte pixels of group g: four as one streaming 16-byte store, the two of a width % 4 == 2 tail (!full) as 8 bytes;
 * store = the group is inside the row.  px3 (wave-uniform, MIBAYER_FLAG_DST_24BIT): byte 3 of every pixel is dropped --
 * the layouts are RGBx / BGRx, so three fixed v_perm_b32 close the gaps -- and the group is 12 bytes at out + 12 g, one
 * streaming store; the tail is 6 bytes, a dword and a 16-bit store, and not a byte more (the row may end there) */
__device__ __forceinline__ void store_strip8 (uint8_t *out, int g, bool store, bool full, bool px3, u32x4 v)
{
  if (store && px3) {
    uint8_t *q = out + 12 * (size_t) g;
    const uint32_t d0 = __builtin_amdgcn_perm (v.y, v.x, 0x04020100u);
    const uint32_t d1 = __builtin_amdgcn_perm (v.z, v.y, 0x05040201u);
    if (full) {
      const u32x3_a4 three = { d0, d1, __builtin_amdgcn_perm (v.w, v.z, 0x06050402u) };
      __builtin_nontemporal_store (three, (u32x3_a4 *) q);
    } else {
      __builtin_nontemporal_store (d0, (uint32_t *) q);
      __builtin_nontemporal_store ((uint16_t) d1, (uint16_t *) (q + 4));
    }
  } else if (store) {
    uint8_t *q = out + 16 * (size_t) g;
    if (full) {
      __builtin_nontemporal_store (v, (u32x4_a4 *) q);
    } else {
      const u32x2_a4 two = { v.x, v.y };
      __builtin_nontemporal_store (two, (u32x2_a4 *) q);
    }
  }
}

/* byte K of each of x[0..3] as one dword: the plane dword of a channel whose four values sit in byte K */
template <int K>
__device__ __forceinline__ uint32_t gather_byte (const uint32_t (&x)[4])
{
  constexpr uint32_t kSel = 0x0c0c0000u | ((4u + K) << 8) | K;
  return __builtin_amdgcn_perm (x[1], x[0], kSel) | (__builtin_amdgcn_perm (x[3], x[2], kSel) << 16);
}

/* row j of plane k of the frame at dst, as a scalar: read back through v_readfirstlane so that the lane's 32-bit column
 * offset stays apart from it (a store of scalar base + 32-bit lane offset) instead of a 64-bit address per lane and
 * plane.  The address is rebuilt from integers, so it is typed as global memory again (a plain pointer would make the
 * stores flat_store_*) */
typedef __attribute__ ((address_space (1))) uint8_t global_u8;
typedef __attribute__ ((address_space (1))) uint16_t global_u16;
typedef __attribute__ ((address_space (1))) uint32_t global_u32;
__device__ __forceinline__ global_u8 *plane_row (const DeepParams &p, uint8_t *out, int k)
{
  const uint64_t q = (uint64_t) out + (uint64_t) (uint32_t) (k * p.height) * (uint64_t) (uint32_t) p.dst_stride;
  const uint32_t lo = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (uint32_t) q);
  const uint32_t hi = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (uint32_t) (q >> 32));
  return (global_u8 *) (((uint64_t) hi << 32) | lo);
}

/* DeepParams::planar as the row loops read it, once per row: the empty asm keeps the test and the plane bases out of
 * the loops' invariants, so p.planar is the only scalar that lives across a row for them, and the bases cost a few
 * scalar instructions per row (the colour kernel has no scalar register to spare: hoisted, they would be spilled) */
__device__ __forceinline__ int planar_of (const DeepParams &p)
{
  int planes = p.planar;
  asm volatile ("" : "+s" (planes));
  return planes;
}

/* planes of 8-bit samples (planes = planar_of (p) != 0, wave-uniform; MIBAYER_FLAG_DST_PLANAR): out = the row in plane
 * 0; a, b, c = the lane's four samples of operands ka, 1 and kc (DeepParams::planar has their planes), one dword each.
 * Plane k is rows [k * height, (k + 1) * height) of the frame, so a row's base is scalar and the lane adds 4 g: one
 * streaming dword store per plane, 256 contiguous bytes per wave and plane; the two samples of a width % 4 == 2 tail
 * (!full) as a 16-bit store and not a byte more (the next row, or the next plane, may start there); store = the group
 * is inside the row */
__device__ __forceinline__ void store_planes8 (const DeepParams &p, int planes, uint8_t *out, int g, bool store,
    bool full, int ka, int kc, uint32_t a, uint32_t b, uint32_t c)
{
  if (store) {
    uint32_t x = 4u * (uint32_t) g;
    asm volatile ("" : "+v" (x));       /* per row, like the bases: no 64-bit lane offset kept across the rows */
    global_u8 *qa = plane_row (p, out, (planes >> (2 * ka)) & 3) + x;
    global_u8 *qb = plane_row (p, out, (planes >> 2) & 3) + x;
    global_u8 *qc = plane_row (p, out, (planes >> (2 * kc)) & 3) + x;
    if (full) {
      __builtin_nontemporal_store (a, (global_u32 *) qa);
      __builtin_nontemporal_store (b, (global_u32 *) qb);
      __builtin_nontemporal_store (c, (global_u32 *) qc);
    } else {
      __builtin_nontemporal_store ((uint16_t) a, (global_u16 *) qa);
      __builtin_nontemporal_store ((uint16_t) b, (global_u16 *) qb);
      __builtin_nontemporal_store ((uint16_t) c, (global_u16 *) qc);
    }
  }
}

/* 8-byte pixels of group g: v0 = pixels 0,1 and v1 = pixels 2,3.  A lane holds 32 contiguous bytes, so two stores
 * straight from its registers would each fill every other 16 bytes of the wave's 2 KiB.  The four lanes of a quad swap
 * pieces instead (DPP quad_perm): the first store writes the quad's first 64 bytes, the second its last 64, and
 * write-back stores let the L2 join the two halves of a 128-byte line.  4K x 16, 12-bit -> ARGB64: 30 % of peak with
 * streaming stores straight from the registers, 47 % write-back, 41 % swapped + streaming, 50 % swapped + write-back.
 * Every lane of the wave calls this: the DPP moves read lanes whose own group may lie past the row. */
__device__ __forceinline__ void store_strip16 (const DeepParams &p, uint8_t *out, int g, int lane, u32x4 v0, u32x4 v1)
{
  const int k = lane & 3;
  u32x4 s0, s1;
  deep_quad_pieces (v0, v1, k, s0, s1);
  const int qg = g - k;                                 /* first group of the quad */
  const int ga = qg + (k >> 1), gb = qg + 2 + (k >> 1); /* group whose piece k&1 this lane stores */
  if (ga < p.groups && ((k & 1) == 0 || 4 * ga + 4 <= p.width))
    *(u32x4_a4 *) (out + 32 * (size_t) qg + 16 * k) = s0;
  if (gb < p.groups && ((k & 1) == 0 || 4 * gb + 4 <= p.width))
    *(u32x4_a4 *) (out + 32 * (size_t) qg + 64 + 16 * k) = s1;
}

template <bool IN8, bool OUT16>
__global__ void __launch_bounds__ (256)
bayer2rgb_deep_kernel (DeepParams p)
{
  const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (wave >= p.nwaves)
    return;
  const int lane = (int) (threadIdx.x & 63u);
  const uint32_t crow = fastdiv (wave, p.div_tiles_x);
  const uint32_t tx = wave - crow * p.div_tiles_x.d;
  const uint32_t chunk = p.chunk0 + crow;
  const uint32_t frame = fastdiv (chunk, p.div_chunks);
  const int y0 = (int) (chunk - frame * p.div_chunks.d) * kStripRows;
  const int y1 = y0 + kStripRows < p.height ? y0 + kStripRows : p.height;
  const uint8_t *src = p.nlist
      ? kernarg_table_entry<const uint8_t *> (offsetof (DeepParams, src_list), frame) : p.src + frame * p.src_frame_bytes;
  uint8_t *dst = p.nlist
      ? kernarg_table_entry<uint8_t *> (offsetof (DeepParams, dst_list), frame) : p.dst + frame * p.dst_frame_bytes;
  const int g = (int) tx * 64 + lane;
  const bool first = g == 0;
  const int lastmode = g == p.groups - 1 ? ((p.width & 3) ? 2 : 1) : 0;
  const bool store = g < p.groups;
  const bool full = 4 * g + 4 <= p.width;

  /* every source row of the chunk is loaded up front (kStripRows + 2 loads in flight per lane): raw[0] = up(y0),
   * raw[1 + k] = row y0 + k, and the row past the frame is dn(H-1) (rows past a short last chunk are never used) */
  DeepRaw raw[kStripRows + 2];
#pragma unroll
  for (int i = 0; i < kStripRows + 2; i++) {
    const int r = i == 0 ? (y0 == 0 ? 1 : y0 - 1) : y0 + i - 1;
    raw[i] = deep_load<IN8> (p, src, r < p.height ? r : p.dn_last, g, lane);
  }
  DeepLines up = deep_lines<IN8> (p, raw[0], lane, first, lastmode);
  DeepLines cur = deep_lines<IN8> (p, raw[1], lane, first, lastmode);
#pragma unroll
  for (int k = 0; k < kStripRows; k++) {
    const int j = y0 + k;
    if (j >= y1)
      break;
    const DeepLines dn = deep_lines<IN8> (p, raw[k + 2], lane, first, lastmode);
    /* merge (orc:43-92): T = 0 merge_bg, T = 1 merge_gr */
    const bool t = ((j & 1) ^ p.swap_rows) != 0;
    const uint32_t ve_lo = avg16x2 (up.elo, dn.elo), ve_hi = avg16x2 (up.ehi, dn.ehi);
    const uint32_t vo_lo = avg16x2 (up.olo, dn.olo), vo_hi = avg16x2 (up.ohi, dn.ohi);
    uint32_t rb_lo, rb_hi, b_lo, b_hi, g_lo, g_hi;      /* R', B', G per pixel pair */
    if (t) {
      b_lo = ve_lo;
      b_hi = ve_hi;
      rb_lo = cur.olo;
      rb_hi = cur.ohi;
      g_lo = bsel (kLowHalves, cur.elo, avg16x2 (vo_lo, cur.elo));
      g_hi = bsel (kLowHalves, cur.ehi, avg16x2 (vo_hi, cur.ehi));
    } else {
      b_lo = cur.elo;
      b_hi = cur.ehi;
      rb_lo = vo_lo;
      rb_hi = vo_hi;
      g_lo = bsel (kLowHalves, avg16x2 (ve_lo, cur.olo), cur.olo);
      g_hi = bsel (kLowHalves, avg16x2 (ve_hi, cur.ohi), cur.ohi);
    }
    uint8_t *out = dst + (size_t) j * (size_t) p.dst_stride;
    if constexpr (OUT16) {
      const int s = p.out_shift;
      rb_lo <<= s; rb_hi <<= s; b_lo <<= s; b_hi <<= s; g_lo <<= s; g_hi <<= s;
      /* M_k = [R'_k, B'_k] */
      const uint32_t m0 = __builtin_amdgcn_perm (b_lo, rb_lo, 0x05040100u);
      const uint32_t m1 = __builtin_amdgcn_perm (b_lo, rb_lo, 0x07060302u);
      const uint32_t m2 = __builtin_amdgcn_perm (b_hi, rb_hi, 0x05040100u);
      const uint32_t m3 = __builtin_amdgcn_perm (b_hi, rb_hi, 0x07060302u);
      u32x4 v0, v1;
      v0.x = __builtin_amdgcn_perm (m0, g_lo, p.sel16[0][0]);
      v0.y = __builtin_amdgcn_perm (m0, g_lo, p.sel16[0][1]);
      v0.z = __builtin_amdgcn_perm (m1, g_lo, p.sel16[1][0]);
      v0.w = __builtin_amdgcn_perm (m1, g_lo, p.sel16[1][1]);
      v1.x = __builtin_amdgcn_perm (m2, g_hi, p.sel16[0][0]);
      v1.y = __builtin_amdgcn_perm (m2, g_hi, p.sel16[0][1]);
      v1.z = __builtin_amdgcn_perm (m3, g_hi, p.sel16[1][0]);
      v1.w = __builtin_amdgcn_perm (m3, g_hi, p.sel16[1][1]);
      store_strip16 (p, out, g, lane, v0, v1);
    } else {
      const int s = p.out_shift;
      constexpr uint32_t kLowBytes = 0x00ff00ffu;
      rb_lo = (rb_lo >> s) & kLowBytes; rb_hi = (rb_hi >> s) & kLowBytes;
      b_lo = (b_lo >> s) & kLowBytes; b_hi = (b_hi >> s) & kLowBytes;
      g_lo = (g_lo >> s) & kLowBytes; g_hi = (g_hi >> s) & kLowBytes;
      /* the 8-bit kernel's operands: M = [r' b' r' b'] of a pixel pair, G = green of pixels 0..3 */
      const uint32_t m_lo = rb_lo | (b_lo << 8);
      const uint32_t m_hi = rb_hi | (b_hi << 8);
      const uint32_t gw = __builtin_amdgcn_perm (g_hi, g_lo, 0x06040200u);
      if (const int planes = planar_of (p)) {   /* gw is the green plane's dword; R', B' are M's even, odd bytes */
        store_planes8 (p, planes, out, g, store, full, 0, 2, __builtin_amdgcn_perm (m_hi, m_lo, 0x06040200u), gw,
            __builtin_amdgcn_perm (m_hi, m_lo, 0x07050301u));
      } else {
        u32x4 v;
        v.x = __builtin_amdgcn_perm (m_lo, gw, p.sel[0]);
        v.y = __builtin_amdgcn_perm (m_lo, gw, p.sel[1]);
        v.z = __builtin_amdgcn_perm (m_hi, gw, p.sel[2]);
        v.w = __builtin_amdgcn_perm (m_hi, gw, p.sel[3]);
        store_strip8 (out, g, store, full, p.px3 != 0, v);
      }
    }
    up = cur;
    cur = dn;
  }
}

/* ------------------------------------------------------------------------- */
/* Malvar-He-Cutler demosaic (MIBAYER_FLAG_MHC)                                */
/* ------------------------------------------------------------------------- */
/* Gradient-corrected linear interpolation (Malvar, He, Cutler, ICASSP 2004) on a 5x5 stencil, the filters scaled by
 * 16 to integers, int32 sums, v = clamp ((acc + 8) >> 4, 0, 2^depth - 1), reflect-101 borders (-1 -> 1, -2 -> 2,
 * W -> W-2, W+1 -> W-3, rows alike).  With c = S(y,x), h1 / h2 = the sums of the samples 1 / 2 columns left and right,
 * v1 / v2 the same above and below, d = the four diagonal neighbours:
 *   green at an R / B site      F_G    = 8c + 4(h1 + v1) - 2(h2 + v2)
 *   the row colour at a G site  F_row  = 10c + 8h1 - 2h2 - 2d + v2
 *   the column colour there     F_col  = 10c + 8v1 - 2v2 - 2d + h2
 *   B at R / R at B             F_diag = 12c + 4d - 3(h2 + v2)
 * Per row the non-green site colour is C (R in a red row, B in a blue one) and the other one D: a non-green site is
 * C = S, G = F_G, D = F_diag; a green site G = S, C = F_row, D = F_col.  Which of C / D is R is a property of the row,
 * so it only picks the output selectors (DeepParams::sel_cgd).  Samples and output conversion are the deep path's.
 *
 * Shape: the deep kernel's.  A lane owns 4 pixels, a wave a strip of 256 pixels x kStripRows rows; it loads all
 * kStripRows + 4 source rows first, then walks down with a 5-row window of unpacked rows in registers.  Columns x0-2,
 * x0-1 and x0+4, x0+5 come from the adjacent lanes by DPP (lanes 0 and 63 load their own edge dword), the border
 * columns are reflected in the lanes that hold them. */

/* one source row as the stencil needs it, pixel k = x0 + k: the sample, the sum of its +-1 neighbours, of its +-2 */
struct MhcRow { int c[4], h1[4], h2[4]; };

template <bool IN8>
__device__ __forceinline__ MhcRow mhc_row (const DeepParams &p, const DeepRaw &raw, int lane, bool first, int lastmode)
{
  const bool partial = lastmode == 2;
  uint32_t lo, hi, e;           /* samples as two 16-bit halves: [x0, x0+1], [x0+2, x0+3], the edge pair */
  if constexpr (IN8) {
    lo = __builtin_amdgcn_perm (raw.a, raw.a, 0x0c010c00u);
    hi = __builtin_amdgcn_perm (raw.a, raw.a, 0x0c030c02u);
    e = __builtin_amdgcn_perm (raw.e, raw.e, lane == 0 ? 0x0c030c02u : 0x0c010c00u);
  } else {
    const uint32_t a = partial ? raw.b : raw.a;
    lo = __builtin_amdgcn_perm (a, a, p.in_sel) & p.mask2;
    hi = partial ? 0u : __builtin_amdgcn_perm (raw.b, raw.b, p.in_sel) & p.mask2;
    e = __builtin_amdgcn_perm (raw.e, raw.e, p.in_sel) & p.mask2;
  }
  uint32_t q[4];
  q[0] = from_lane_below (e, hi);                       /* [x0-2, x0-1] */
  q[1] = lo;
  q[2] = hi;
  q[3] = from_lane_above (e, lo);                       /* [x0+4, x0+5] */
  /* reflect-101 at the borders */
  if (first)
    q[0] = bsel (kLowHalves, q[2], q[1]);               /* S(-2) = S(2), S(-1) = S(1) */
  if (lastmode == 1)
    q[3] = bsel (kLowHalves, q[2], q[1]);               /* x0 = W-4: S(W) = S(W-2), S(W+1) = S(W-3) */
  if (partial)
    q[2] = bsel (kLowHalves, q[1], q[0]);               /* x0 = W-2: S(W) = S(W-2), S(W+1) = S(W-3) */
  int s[8];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    s[2 * i] = (int) (q[i] & 0xffffu);
    s[2 * i + 1] = (int) (q[i] >> 16);
  }
  MhcRow r;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    r.c[k] = s[k + 2];
    r.h1[k] = s[k + 1] + s[k + 3];
    r.h2[k] = s[k] + s[k + 4];
  }
  return r;
}

/* pixel k of the centre row z; returns C, G, D at output depth */
template <bool GREEN>
__device__ __forceinline__ void mhc_pixel (const DeepParams &p, const MhcRow &m2, const MhcRow &m1, const MhcRow &z,
    const MhcRow &p1, const MhcRow &p2, int k, int &C, int &G, int &D)
{
  const int c = z.c[k];
  const int h1 = z.h1[k], h2 = z.h2[k];
  const int v1 = m1.c[k] + p1.c[k];
  const int v2 = m2.c[k] + p2.c[k];
  const int d = m1.h1[k] + p1.h1[k];
  int f1, f2;
  if constexpr (GREEN) {
    G = c;
    f1 = 10 * c + 8 * h1 - 2 * (h2 + d) + v2;           /* C = F_row */
    f2 = 10 * c + 8 * v1 - 2 * (v2 + d) + h2;           /* D = F_col */
  } else {
    C = c;
    f1 = 8 * c + 4 * (h1 + v1) - 2 * (h2 + v2);         /* G = F_G */
    f2 = 12 * c + 4 * d - 3 * (h2 + v2);                /* D = F_diag */
  }
  f1 = min (max ((f1 + 8) >> 4, 0), p.vmax);         /* v_med3_i32 */
  f2 = min (max ((f2 + 8) >> 4, 0), p.vmax);
  if constexpr (GREEN)
    C = f1;
  else
    G = f1;
  D = f2;
}

/* reflect-101 row index of a frame of `height` rows (-1 -> 1, -2 -> 2, H -> H-2, H+1 -> H-3); rows further out are
 * never used and map to H-1 */
__device__ __forceinline__ int reflect_row (int r, int height)
{
  r = r < 0 ? -r : r;
  return r > height + 1 ? height - 1 : r >= height ? 2 * height - 2 - r : r;
}

/* {x = [C, G], y = [D, 0]} of the lane's four pixels at output depth -> output pixels by v_perm_b32 with the selectors
 * s0, s1 (DeepParams::sel_cgd): 8-byte pixels v0 = pixels 0,1 and v1 = pixels 2,3 (s0 / s1 = the two dwords of a
 * pixel), 4-byte pixels v0 = all four (s0 only, v1 is not written) */
template <bool OUT16>
__device__ __forceinline__ void emit_cgd (const uint32_t (&x)[4], const uint32_t (&y)[4], uint32_t s0, uint32_t s1,
    u32x4 &v0, u32x4 &v1)
{
  if constexpr (OUT16) {
    v0.x = __builtin_amdgcn_perm (x[0], y[0], s0);
    v0.y = __builtin_amdgcn_perm (x[0], y[0], s1);
    v0.z = __builtin_amdgcn_perm (x[1], y[1], s0);
    v0.w = __builtin_amdgcn_perm (x[1], y[1], s1);
    v1.x = __builtin_amdgcn_perm (x[2], y[2], s0);
    v1.y = __builtin_amdgcn_perm (x[2], y[2], s1);
    v1.z = __builtin_amdgcn_perm (x[3], y[3], s0);
    v1.w = __builtin_amdgcn_perm (x[3], y[3], s1);
  } else {
    v0.x = __builtin_amdgcn_perm (x[0], y[0], s0);
    v0.y = __builtin_amdgcn_perm (x[1], y[1], s0);
    v0.z = __builtin_amdgcn_perm (x[2], y[2], s0);
    v0.w = __builtin_amdgcn_perm (x[3], y[3], s0);
  }
}

template <bool IN8, bool OUT16>
__global__ void __launch_bounds__ (256)
bayer2rgb_mhc_kernel (DeepParams p)
{
  const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (wave >= p.nwaves)
    return;
  const int lane = (int) (threadIdx.x & 63u);
  const uint32_t crow = fastdiv (wave, p.div_tiles_x);
  const uint32_t tx = wave - crow * p.div_tiles_x.d;
  const uint32_t chunk = p.chunk0 + crow;
  const uint32_t frame = fastdiv (chunk, p.div_chunks);
  const int y0 = (int) (chunk - frame * p.div_chunks.d) * kStripRows;
  const int y1 = y0 + kStripRows < p.height ? y0 + kStripRows : p.height;
  const uint8_t *src = p.nlist
      ? kernarg_table_entry<const uint8_t *> (offsetof (DeepParams, src_list), frame) : p.src + frame * p.src_frame_bytes;
  uint8_t *dst = p.nlist
      ? kernarg_table_entry<uint8_t *> (offsetof (DeepParams, dst_list), frame) : p.dst + frame * p.dst_frame_bytes;
  const int g = (int) tx * 64 + lane;
  const bool first = g == 0;
  const int lastmode = g == p.groups - 1 ? ((p.width & 3) ? 2 : 1) : 0;
  const bool store = g < p.groups;
  const bool full = 4 * g + 4 <= p.width;

  /* raw[i] = row y0 - 2 + i, reflected; rows past y1 + 1 (a short last chunk) are never used and read row H-1 */
  DeepRaw raw[kStripRows + 4];
#pragma unroll
  for (int i = 0; i < kStripRows + 4; i++)
    raw[i] = deep_load<IN8> (p, src, reflect_row (y0 - 2 + i, p.height), g, lane);
  MhcRow w0 = mhc_row<IN8> (p, raw[0], lane, first, lastmode);
  MhcRow w1 = mhc_row<IN8> (p, raw[1], lane, first, lastmode);
  MhcRow w2 = mhc_row<IN8> (p, raw[2], lane, first, lastmode);
  MhcRow w3 = mhc_row<IN8> (p, raw[3], lane, first, lastmode);
#pragma unroll
  for (int k = 0; k < kStripRows; k++) {
    const int j = y0 + k;
    if (j >= y1)
      break;
    const MhcRow w4 = mhc_row<IN8> (p, raw[k + 4], lane, first, lastmode);
    int C[4], G[4], D[4];
    if (((j & 1) ^ p.green_odd) == 0) {             /* green at even columns (x0 is even) */
      mhc_pixel<true> (p, w0, w1, w2, w3, w4, 0, C[0], G[0], D[0]);
      mhc_pixel<false> (p, w0, w1, w2, w3, w4, 1, C[1], G[1], D[1]);
      mhc_pixel<true> (p, w0, w1, w2, w3, w4, 2, C[2], G[2], D[2]);
      mhc_pixel<false> (p, w0, w1, w2, w3, w4, 3, C[3], G[3], D[3]);
    } else {
      mhc_pixel<false> (p, w0, w1, w2, w3, w4, 0, C[0], G[0], D[0]);
      mhc_pixel<true> (p, w0, w1, w2, w3, w4, 1, C[1], G[1], D[1]);
      mhc_pixel<false> (p, w0, w1, w2, w3, w4, 2, C[2], G[2], D[2]);
      mhc_pixel<true> (p, w0, w1, w2, w3, w4, 3, C[3], G[3], D[3]);
    }
    const int rk = (j & 1) ^ p.red_odd;             /* 0: C is R (red row), 1: C is B */
    const int s = p.out_shift;
    uint32_t x[4], y[4];                                /* x = [C, G], y = [D, 0] at output depth */
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if constexpr (OUT16) {
        x[i] = ((uint32_t) C[i] << s) | ((uint32_t) G[i] << (16 + s));
        y[i] = (uint32_t) D[i] << s;
      } else {
        x[i] = ((uint32_t) C[i] >> s) | (((uint32_t) G[i] >> s) << 16);
        y[i] = (uint32_t) D[i] >> s;
      }
    }
    uint8_t *out = dst + (size_t) j * (size_t) p.dst_stride;
    if constexpr (OUT16) {
      const uint32_t s0 = p.sel_cgd[rk][0], s1 = p.sel_cgd[rk][1];
      u32x4 v0, v1;
      emit_cgd<true> (x, y, s0, s1, v0, v1);
      store_strip16 (p, out, g, lane, v0, v1);
    } else if (const int planes = planar_of (p)) {      /* C, G, D: bytes 0, 2 of x, 0 of y; C is R in a red row */
      store_planes8 (p, planes, out, g, store, full, rk ? 2 : 0, rk ? 0 : 2, gather_byte<0> (x), gather_byte<2> (x),
          gather_byte<0> (y));
    } else {
      const uint32_t s0 = p.sel_cgd[rk][0];
      u32x4 v, unused;
      emit_cgd<false> (x, y, s0, s0, v, unused);
      store_strip8 (out, g, store, full, p.px3 != 0, v);
    }
    w0 = w1;
    w1 = w2;
    w2 = w3;
    w3 = w4;
  }
}

/* ------------------------------------------------------------------------- */
/* fused colour stage (MIBAYER_FLAG_COLOUR)                                    */
/* ------------------------------------------------------------------------- */
/* Black level, Q12 colour matrix and tone curve (include/mibayer.h) on the demosaiced values while they are still
 * integers in registers: no second pass over a 4- or 8-byte-per-pixel frame.  The rows go through the MHC kernel's
 * unpacked window (mhc_row); R, G, B come from the MHC filters or from the deep path's bilinear closed form, which
 * on that window is, with a = avg of the row's +-1 neighbours and u / d the rows up (j) / dn (j):
 *   non-green site: C = S, G = avg (avg (S_u, S_d), a), D = avg (a_u, a_d);  green site: G = S, C = a, D = avg (S_u, S_d)
 * (C the row's own colour, D the other one, as in the MHC kernel).  Reflect-101 columns give the reference's edge
 * columns O[0] = S[1] and E[W-1] = S[W-2]; O[W-2] = S[W-3] is patched into the row (colour_row), and row H stands for
 * dn (H-1) = dn_last instead of the reflected H-2.
 *
 * One kernel, no template fan-out: method, sample width, output width and tone curve are uniform run-time branches,
 * and the row loop is rolled -- the window rotates through registers and the loads run kColourAhead rows ahead of it --
 * which keeps the code a fraction of the four unrolled MHC kernels' (the library has a size cap; DESIGN.md 3b has what
 * the rolled loop costs).  The tone table (257 dwords) is copied from the kernel
 * arguments to LDS by the whole workgroup BEFORE the waves beyond the launch leave: no wave skips the barrier. */

constexpr int kColourAhead = 4;

/* row r of the frame, mapped into it: reflect-101 for the MHC filters, the reference's up () / dn () for bilinear */
__device__ __forceinline__ DeepRaw colour_load (const ColourParams &cp, const uint8_t *src, int r, int g, int lane)
{
  const DeepParams &p = cp.d;
  if (cp.mhc) {
    r = reflect_row (r, p.height);
  } else {
    r = r < 0 ? -r : r;
    r = r == p.height ? p.dn_last : r > p.height ? p.height - 1 : r;
  }
  if (cp.in8)
    return deep_load<true> (p, src, r, g, lane);
  return deep_load<false> (p, src, r, g, lane);
}

__device__ __forceinline__ MhcRow colour_row (const ColourParams &cp, const DeepRaw &raw, int lane, bool first,
    int lastmode)
{
  MhcRow r;
  if (cp.in8)
    r = mhc_row<true> (cp.d, raw, lane, first, lastmode);
  else
    r = mhc_row<false> (cp.d, raw, lane, first, lastmode);
  if (!cp.mhc) {
    /* O[W-2] = S[W-3] (gstbayer2rgb.c:354-381): h2 of pixel W-1 is S[W-3] + S(W+1) = 2 S[W-3] by the reflection */
    if (lastmode == 1)
      r.h1[2] = r.h2[3];
    if (lastmode == 2)
      r.h1[0] = r.h2[1];
  }
  return r;
}

__device__ __forceinline__ int avg_i (int a, int b)
{
  return (a + b + 1) >> 1;
}

/* the deep path's bilinear values of pixel k of row z between rows u = up (j) and d = dn (j) */
template <bool GREEN>
__device__ __forceinline__ void bilinear_pixel (const MhcRow &u, const MhcRow &z, const MhcRow &d, int k, int &C, int &G,
    int &D)
{
  const int a = (z.h1[k] + 1) >> 1;
  const int vc = avg_i (u.c[k], d.c[k]);
  if constexpr (GREEN) {
    G = z.c[k];
    C = a;
    D = vc;
  } else {
    C = z.c[k];
    G = avg_i (vc, a);
    D = avg_i ((u.h1[k] + 1) >> 1, (d.h1[k] + 1) >> 1);
  }
}

__global__ void __launch_bounds__ (256)
bayer2rgb_colour_kernel (ColourParams cp)
{
  __shared__ uint32_t tone[257];
  const DeepParams &p = cp.d;
  if (cp.s.has_tone) {
    /* kernarg_table_entry at a per-lane index: not the scalar load its other users get, a vector load from the
     * constant address space -- 257 dwords once per workgroup */
    constexpr size_t kToneOffset = offsetof (ColourParams, s) + offsetof (ColourStage, tone);
    tone[threadIdx.x] = kernarg_table_entry<uint32_t> (kToneOffset, threadIdx.x);
    if (threadIdx.x == 0)
      tone[256] = kernarg_table_entry<uint32_t> (kToneOffset, 256);
    __syncthreads ();
  }
  const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (wave >= p.nwaves)
    return;
  const int lane = (int) (threadIdx.x & 63u);
  const uint32_t crow = fastdiv (wave, p.div_tiles_x);
  const uint32_t tx = wave - crow * p.div_tiles_x.d;
  const uint32_t chunk = p.chunk0 + crow;
  const uint32_t frame = fastdiv (chunk, p.div_chunks);
  const int y0 = (int) (chunk - frame * p.div_chunks.d) * kStripRows;
  const int y1 = y0 + kStripRows < p.height ? y0 + kStripRows : p.height;
  const uint8_t *src = p.nlist
      ? kernarg_table_entry<const uint8_t *> (offsetof (DeepParams, src_list), frame) : p.src + frame * p.src_frame_bytes;
  uint8_t *dst = p.nlist
      ? kernarg_table_entry<uint8_t *> (offsetof (DeepParams, dst_list), frame) : p.dst + frame * p.dst_frame_bytes;
  const int g = (int) tx * 64 + lane;
  const bool first = g == 0;
  const int lastmode = g == p.groups - 1 ? ((p.width & 3) ? 2 : 1) : 0;
  const bool store = g < p.groups;
  const bool full = 4 * g + 4 <= p.width;
  const int s = p.out_shift;
  const int tshift = cp.out16 ? s : 8 - s;              /* 16 - depth */

  /* rows y0-2 .. y0+1 fill the window, rows y0+2 .. run kColourAhead loads ahead of it */
  MhcRow w0, w1, w2, w3;
  DeepRaw ring[kColourAhead];
  {
    DeepRaw head[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
      head[i] = colour_load (cp, src, y0 - 2 + i, g, lane);
#pragma unroll
    for (int i = 0; i < kColourAhead; i++)
      ring[i] = colour_load (cp, src, y0 + 2 + i, g, lane);
    w0 = colour_row (cp, head[0], lane, first, lastmode);
    w1 = colour_row (cp, head[1], lane, first, lastmode);
    w2 = colour_row (cp, head[2], lane, first, lastmode);
    w3 = colour_row (cp, head[3], lane, first, lastmode);
  }
#pragma unroll 1
  for (int j = y0; j < y1; j++) {
    const MhcRow w4 = colour_row (cp, ring[0], lane, first, lastmode);
#pragma unroll
    for (int i = 0; i + 1 < kColourAhead; i++)
      ring[i] = ring[i + 1];
    if (j + 2 + kColourAhead <= y1 + 1)                 /* the last output row, y1 - 1, needs row y1 + 1 */
      ring[kColourAhead - 1] = colour_load (cp, src, j + 2 + kColourAhead, g, lane);
    int C[4], G[4], D[4];
    const bool green_even = ((j & 1) ^ p.green_odd) == 0;
    if (cp.mhc) {
      if (green_even) {
        mhc_pixel<true> (p, w0, w1, w2, w3, w4, 0, C[0], G[0], D[0]);
        mhc_pixel<false> (p, w0, w1, w2, w3, w4, 1, C[1], G[1], D[1]);
        mhc_pixel<true> (p, w0, w1, w2, w3, w4, 2, C[2], G[2], D[2]);
        mhc_pixel<false> (p, w0, w1, w2, w3, w4, 3, C[3], G[3], D[3]);
      } else {
        mhc_pixel<false> (p, w0, w1, w2, w3, w4, 0, C[0], G[0], D[0]);
        mhc_pixel<true> (p, w0, w1, w2, w3, w4, 1, C[1], G[1], D[1]);
        mhc_pixel<false> (p, w0, w1, w2, w3, w4, 2, C[2], G[2], D[2]);
        mhc_pixel<true> (p, w0, w1, w2, w3, w4, 3, C[3], G[3], D[3]);
      }
    } else if (green_even) {
      bilinear_pixel<true> (w1, w2, w3, 0, C[0], G[0], D[0]);
      bilinear_pixel<false> (w1, w2, w3, 1, C[1], G[1], D[1]);
      bilinear_pixel<true> (w1, w2, w3, 2, C[2], G[2], D[2]);
      bilinear_pixel<false> (w1, w2, w3, 3, C[3], G[3], D[3]);
    } else {
      bilinear_pixel<false> (w1, w2, w3, 0, C[0], G[0], D[0]);
      bilinear_pixel<true> (w1, w2, w3, 1, C[1], G[1], D[1]);
      bilinear_pixel<false> (w1, w2, w3, 2, C[2], G[2], D[2]);
      bilinear_pixel<true> (w1, w2, w3, 3, C[3], G[3], D[3]);
    }
    /* the colour stage: (R, G, B) -> black level -> matrix -> clamp, 24-bit multiplies on the split entries */
    const bool c_is_red = ((j & 1) ^ p.red_odd) == 0;
    int v[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = max ((c_is_red ? C[i] : D[i]) - cp.s.black[0], 0);
      const int gr = max (G[i] - cp.s.black[1], 0);
      const int b = max ((c_is_red ? D[i] : C[i]) - cp.s.black[2], 0);
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const int hi = __mul24 (cp.s.m_hi[3 * ch], r) + __mul24 (cp.s.m_hi[3 * ch + 1], gr)
            + __mul24 (cp.s.m_hi[3 * ch + 2], b);
        const uint32_t lo = __umul24 ((uint32_t) cp.s.m_lo[3 * ch], (uint32_t) r)
            + __umul24 ((uint32_t) cp.s.m_lo[3 * ch + 1], (uint32_t) gr)
            + __umul24 ((uint32_t) cp.s.m_lo[3 * ch + 2], (uint32_t) b);
        v[i][ch] = min (max (hi + (int) ((lo + 2048u) >> 12), 0), p.vmax);
      }
    }
    uint32_t o[4][3];
    if (cp.s.has_tone) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          const uint32_t t = (uint32_t) v[i][ch] << tshift;
          const uint32_t ti = t >> 8, tf = t & 255u;
          const uint32_t q = min ((__umul24 (tone[ti], 256u - tf) + __umul24 (tone[ti + 1], tf) + 128u) >> 8, 65535u);
          o[i][ch] = cp.out16 ? q : q >> 8;
        }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
          o[i][ch] = cp.out16 ? (uint32_t) v[i][ch] << s : (uint32_t) v[i][ch] >> s;
    }
    /* the MHC kernel's packing and stores with C = R, D = B: x = [R, G], y = [B, 0] */
    uint32_t x[4], y[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      x[i] = o[i][0] | (o[i][1] << 16);
      y[i] = o[i][2];
    }
    uint8_t *out = dst + (size_t) j * (size_t) p.dst_stride;
    const uint32_t s0 = p.sel_cgd[0][0], s1 = p.sel_cgd[0][1];
    if (cp.out16) {
      u32x4 v0, v1;
      emit_cgd<true> (x, y, s0, s1, v0, v1);
      store_strip16 (p, out, g, lane, v0, v1);
    } else if (const int planes = planar_of (p)) {
      store_planes8 (p, planes, out, g, store, full, 0, 2, gather_byte<0> (x), gather_byte<2> (x), gather_byte<0> (y));
    } else {
      u32x4 vv, unused;
      emit_cgd<false> (x, y, s0, s0, vv, unused);
      store_strip8 (out, g, store, full, p.px3 != 0, vv);
    }
    w0 = w1;
    w1 = w2;
    w2 = w3;
    w3 = w4;
  }
}

/* ------------------------------------------------------------------------- */
/* strip launcher                                                              */
/* ------------------------------------------------------------------------- */
/* the launch-dependent fields of q (strips of 256 pixels x kStripRows-row chunks, chunks [chunk0, chunk0 + nchunks) of the
 * batch, nchunks < 0: all) and the grid; *grid = 0: nothing to launch */
static hipError_t deep_grid (DeepParams &q, int nframes, long long chunk0, long long nchunks, unsigned *grid)
{
  *grid = 0;
  q.groups = (q.width + 3) / 4;
  const int tiles_x = (q.groups + 63) / 64;
  const long long chunks_per_frame = (q.height + kStripRows - 1) / kStripRows;
  const long long frames = q.nlist > 0 ? q.nlist : nframes;
  if (q.nlist > kMaxList || frames <= 0)
    return frames == 0 ? hipSuccess : hipErrorInvalidValue;
  const long long total = frames * chunks_per_frame;
  if (nchunks < 0) {
    chunk0 = 0;
    nchunks = total;
  }
  if (chunk0 < 0 || chunk0 + nchunks > total)
    return hipErrorInvalidValue;
  if (nchunks == 0)
    return hipSuccess;
  const long long waves = nchunks * tiles_x;
  if (total > 0x7fffffffLL || waves > 0x7fffffffLL)
    return hipErrorInvalidValue;
  q.div_tiles_x = make_fastdiv ((uint32_t) tiles_x);
  q.div_chunks = make_fastdiv ((uint32_t) chunks_per_frame);
  q.chunk0 = (uint32_t) chunk0;
  q.nwaves = (uint32_t) waves;
  *grid = (unsigned) ((waves + 3) / 4);
  return hipSuccess;
}

typedef void (*StripFn) (DeepParams);
/* [mhc][in8][out16]; bilinear 8 -> 8 is the production (LDS) kernels' unless the pixels are 3 bytes (px3) or the output
 * is planes (planar) */
static const StripFn kStripKernels[2][2][2] = {
  { { bayer2rgb_deep_kernel<false, false>, bayer2rgb_deep_kernel<false, true> },
    { bayer2rgb_deep_kernel<true, false>, bayer2rgb_deep_kernel<true, true> } },
  { { bayer2rgb_mhc_kernel<false, false>, bayer2rgb_mhc_kernel<false, true> },
    { bayer2rgb_mhc_kernel<true, false>, bayer2rgb_mhc_kernel<true, true> } },
};

hipError_t launch_strip (const DeepParams &p, StripKind kind, const ColourStage *stage, int nframes, hipStream_t stream,
    long long chunk0, long long nchunks)
{
  const StripFn fn = kStripKernels[kind.mhc][kind.in8][kind.out16];
  if (p.width < 4 || p.height < 3 || (p.width & 1) || ((p.px3 || p.planar) && kind.out16)
      || (p.px3 && p.planar))
    return hipErrorInvalidValue;
  if (!stage && !kind.mhc && kind.in8 && !kind.out16 && !p.px3 && !p.planar)        /* the production kernels' */
    return hipErrorInvalidValue;
  ColourParams q;               /* q.d alone is the argument of the plain kernels */
  q.d = p;
  unsigned grid = 0;
  const hipError_t e = deep_grid (q.d, nframes, chunk0, nchunks, &grid);
  if (e != hipSuccess || grid == 0)
    return e;
  if (stage) {
    q.mhc = kind.mhc;
    q.in8 = kind.in8;
    q.out16 = kind.out16;
    q.s = *stage;
    hipLaunchKernelGGL (bayer2rgb_colour_kernel, dim3 (grid), dim3 (256), 0, stream, q);
  } else {
    hipLaunchKernelGGL (fn, dim3 (grid), dim3 (256), 0, stream, q.d);
  }
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* half-size demosaic (MIBAYER_FLAG_HALF)                                      */
/* ------------------------------------------------------------------------- */
/* One output pixel per CFA quad (include/mibayer.h, group `half`): R and B are the quad's own samples, G the rounded
 * mean of its two greens at native depth; then the colour stage (optional) and the deep path's output conversion and
 * layouts.  Pointwise: no neighbourhood, no halo, no border rule, no LDS but the stage's tone table.
 *
 * Shape: a lane owns 4 output pixels = 8 source columns of two rows (one 8-byte load per row from an 8-bit mosaic, one
 * 16-byte load from 16-bit words; rows need only be dword-aligned), a wave a strip of kHalfWavePixels output pixels x
 * kHalfRows output rows.  It issues all 2 kHalfRows row loads up front, then walks down in a ROLLED loop -- the rows
 * rotate through the registers -- so that the stage and the three store families exist once in the code (the library
 * has a size cap).  One kernel: sample width, output format and the stage are uniform run-time branches.  A row's last
 * lane may hold 1, 2 or 3 pixels (OW may be odd): its loads stay inside the row's samples and its stores write exactly
 * px * n bytes -- the next row, or the next plane, may start right behind them. */

struct HalfRaw { uint32_t w[4]; };      /* 8-bit mosaic: w[0], w[1] = columns 0..3, 4..7; words: w[i] = columns 2i, 2i+1 */

/* the lane's samples of one mosaic row; n = its output pixels (<= 0: none).  FULL (wave-uniform: every lane of the wave
 * has n = 4): one load, nothing masked; else dword by dword -- 2 n columns are read and not a dword more */
template <bool FULL>
__device__ __forceinline__ HalfRaw half_load (bool in8, const uint8_t *row, int g, int n)
{
  HalfRaw r = { { 0u, 0u, 0u, 0u } };
  if (in8) {
    const uint8_t *q = row + 8 * (size_t) g;
    if constexpr (FULL) {
      const u32x2_a4 c = __builtin_nontemporal_load ((const u32x2_a4 *) q);
      r.w[0] = c.x;
      r.w[1] = c.y;
    } else {
#pragma unroll
      for (int i = 0; i < 2; i++)
        if (2 * i < n)
          r.w[i] = *(const uint32_t *) (q + 4 * i);
    }
  } else {
    const uint8_t *q = row + 16 * (size_t) g;
    if constexpr (FULL) {
      const u32x4_a4 c = __builtin_nontemporal_load ((const u32x4_a4 *) q);
      r.w[0] = c.x;
      r.w[1] = c.y;
      r.w[2] = c.z;
      r.w[3] = c.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (i < n)
          r.w[i] = *(const uint32_t *) (q + 4 * i);
    }
  }
  return r;
}

/* the two samples of output pixel i in one row as [left | right << 16], masked, in host byte order */
__device__ __forceinline__ void half_pairs (const HalfParams &hp, const HalfRaw &r, uint32_t (&x)[4])
{
  if (hp.in8) {
    x[0] = __builtin_amdgcn_perm (r.w[0], r.w[0], 0x0c010c00u);
    x[1] = __builtin_amdgcn_perm (r.w[0], r.w[0], 0x0c030c02u);
    x[2] = __builtin_amdgcn_perm (r.w[1], r.w[1], 0x0c010c00u);
    x[3] = __builtin_amdgcn_perm (r.w[1], r.w[1], 0x0c030c02u);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
      x[i] = __builtin_amdgcn_perm (r.w[i], r.w[i], hp.d.in_sel) & hp.d.mask2;
  }
}

/* n (1 .. 4) 4-byte pixels of group g, or 3-byte ones (px3: byte 3 of every pixel dropped, as store_strip8 does) */
__device__ __forceinline__ void half_store8 (uint8_t *out, int g, int n, bool px3, u32x4 v)
{
  if (n <= 0)
    return;
  if (px3) {
    uint8_t *q = out + 12 * (size_t) g;
    const uint32_t d0 = __builtin_amdgcn_perm (v.y, v.x, 0x04020100u);
    const uint32_t d1 = __builtin_amdgcn_perm (v.z, v.y, 0x05040201u);
    const uint32_t d2 = __builtin_amdgcn_perm (v.w, v.z, 0x06050402u);
    if (n >= 4) {
      const u32x3_a4 three = { d0, d1, d2 };
      __builtin_nontemporal_store (three, (u32x3_a4 *) q);
    } else if (n == 3) {                /* 9 bytes */
      const u32x2_a4 two = { d0, d1 };
      __builtin_nontemporal_store (two, (u32x2_a4 *) q);
      __builtin_nontemporal_store ((uint8_t) d2, q + 8);
    } else if (n == 2) {                /* 6 bytes */
      __builtin_nontemporal_store (d0, (uint32_t *) q);
      __builtin_nontemporal_store ((uint16_t) d1, (uint16_t *) (q + 4));
    } else {                            /* 3 bytes */
      __builtin_nontemporal_store ((uint16_t) d0, (uint16_t *) q);
      __builtin_nontemporal_store ((uint8_t) (d0 >> 16), q + 2);
    }
  } else {
    uint8_t *q = out + 16 * (size_t) g;
    if (n >= 4) {
      __builtin_nontemporal_store (v, (u32x4_a4 *) q);
    } else {
      if (n >= 2) {
        const u32x2_a4 two = { v.x, v.y };
        __builtin_nontemporal_store (two, (u32x2_a4 *) q);
      }
      if (n & 1)
        __builtin_nontemporal_store (n == 1 ? v.x : v.z, (uint32_t *) (q + 4 * (n - 1)));
    }
  }
}

/* n (1 .. 4) samples of one plane's row: a dword, or a 16-bit and / or a byte store */
__device__ __forceinline__ void half_plane (global_u8 *q, int n, uint32_t a)
{
  if (n >= 4) {
    __builtin_nontemporal_store (a, (global_u32 *) q);
  } else {
    if (n >= 2)
      __builtin_nontemporal_store ((uint16_t) a, (global_u16 *) q);
    if (n & 1)
      __builtin_nontemporal_store ((uint8_t) (a >> (8 * (n - 1))), q + (n - 1));
  }
}

/* 8-byte pixels: store_strip16's quad exchange (every lane of the wave calls this), with pieces of one pixel where an
 * odd row ends */
__device__ __forceinline__ void half_store16 (const DeepParams &p, uint8_t *out, int g, int lane, u32x4 v0, u32x4 v1)
{
  const int k = lane & 3;
  u32x4 s0, s1;
  deep_quad_pieces (v0, v1, k, s0, s1);
  const int qg = g - k;                                 /* first group of the quad */
  uint8_t *q = out + 32 * (size_t) qg + 16 * k;
  /* pixels of the row from this lane's piece of the quad's first / last 64 bytes on */
  const int ma = p.width - (4 * (qg + (k >> 1)) + 2 * (k & 1)), mb = ma - 8;
  if (ma >= 2) {
    *(u32x4_a4 *) q = s0;
  } else if (ma == 1) {
    const u32x2_a4 one = { s0.x, s0.y };
    *(u32x2_a4 *) q = one;
  }
  if (mb >= 2) {
    *(u32x4_a4 *) (q + 64) = s1;
  } else if (mb == 1) {
    const u32x2_a4 one = { s1.x, s1.y };
    *(u32x2_a4 *) (q + 64) = one;
  }
}

__global__ void __launch_bounds__ (256)
bayer2rgb_half_kernel (HalfParams hp)
{
  __shared__ uint32_t tone[257];
  const DeepParams &p = hp.d;
  const bool has_tone = hp.colour && hp.s.has_tone;
  if (has_tone) {               /* the colour kernel's rule: the whole workgroup copies, no wave leaves before the barrier */
    constexpr size_t kToneOffset = offsetof (HalfParams, s) + offsetof (ColourStage, tone);
    tone[threadIdx.x] = kernarg_table_entry<uint32_t> (kToneOffset, threadIdx.x);
    if (threadIdx.x == 0)
      tone[256] = kernarg_table_entry<uint32_t> (kToneOffset, 256);
    __syncthreads ();
  }
  const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane ((int) (blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (wave >= p.nwaves)
    return;
  const int lane = (int) (threadIdx.x & 63u);
  const uint32_t crow = fastdiv (wave, p.div_tiles_x);
  const uint32_t tx = wave - crow * p.div_tiles_x.d;
  const uint32_t frame = fastdiv (crow, p.div_chunks);
  const int y0 = (int) (crow - frame * p.div_chunks.d) * kHalfRows;
  const int y1 = y0 + kHalfRows < p.height ? y0 + kHalfRows : p.height;
  const uint8_t *src = p.nlist
      ? kernarg_table_entry<const uint8_t *> (offsetof (DeepParams, src_list), frame) : p.src + frame * p.src_frame_bytes;
  uint8_t *dst = p.nlist
      ? kernarg_table_entry<uint8_t *> (offsetof (DeepParams, dst_list), frame) : p.dst + frame * p.dst_frame_bytes;
  const int g = (int) tx * 64 + lane;
  const int left = p.width - kHalfLanePixels * g;       /* output pixels of the row from this lane on */
  const int n = left < kHalfLanePixels ? left : kHalfLanePixels;
  const int s = p.out_shift;
  const int tshift = hp.out16 ? s : 8 - s;              /* 16 - depth */

  /* raw[i] = source row 2 y0 + i; rows past the last quad row (a short last chunk) are never used and read that row.
   * Sample width and "the row ends in this wave" are wave-uniform: a wave inside the row issues 2 kHalfRows plain wide
   * loads back to back */
  HalfRaw raw[2 * kHalfRows];
  const bool wave_full = kHalfWavePixels * ((int) tx + 1) <= p.width;
  const auto load_rows = [&] (auto full, bool in8) {
#pragma unroll
    for (int i = 0; i < 2 * kHalfRows; i++) {
      const int r = 2 * y0 + i < 2 * p.height ? 2 * y0 + i : 2 * p.height - 1;
      raw[i] = half_load<decltype (full)::value> (in8, src + (size_t) r * (size_t) p.src_stride, g, n);
    }
  };
  if (wave_full && hp.in8)
    load_rows (std::true_type (), true);
  else if (wave_full)
    load_rows (std::true_type (), false);
  else if (hp.in8)
    load_rows (std::false_type (), true);
  else
    load_rows (std::false_type (), false);
#pragma unroll 1
  for (int j = y0; j < y1; j++) {
    uint32_t t[4], b[4];
    half_pairs (hp, raw[0], t);
    half_pairs (hp, raw[1], b);
#pragma unroll
    for (int i = 0; i + 2 < 2 * kHalfRows; i++)
      raw[i] = raw[i + 2];
    int v[4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      /* green at the odd column of the top row (bggr, rggb), else the halves change places first */
      const uint32_t tt = p.green_odd ? t[i] : __builtin_amdgcn_alignbit (t[i], t[i], 16);
      const uint32_t bb = p.green_odd ? b[i] : __builtin_amdgcn_alignbit (b[i], b[i], 16);
      const int c_top = (int) (tt & kLowHalves), c_bot = (int) (bb >> 16);
      v[i][0] = p.red_odd ? c_bot : c_top;
      v[i][1] = avg_i ((int) (tt >> 16), (int) (bb & kLowHalves));
      v[i][2] = p.red_odd ? c_top : c_bot;
    }
    if (hp.colour) {            /* the colour kernel's stage: black level -> matrix -> clamp */
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int r = max (v[i][0] - hp.s.black[0], 0);
        const int gr = max (v[i][1] - hp.s.black[1], 0);
        const int bl = max (v[i][2] - hp.s.black[2], 0);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          const int hi = __mul24 (hp.s.m_hi[3 * ch], r) + __mul24 (hp.s.m_hi[3 * ch + 1], gr)
              + __mul24 (hp.s.m_hi[3 * ch + 2], bl);
          const uint32_t lo = __umul24 ((uint32_t) hp.s.m_lo[3 * ch], (uint32_t) r)
              + __umul24 ((uint32_t) hp.s.m_lo[3 * ch + 1], (uint32_t) gr)
              + __umul24 ((uint32_t) hp.s.m_lo[3 * ch + 2], (uint32_t) bl);
          v[i][ch] = min (max (hi + (int) ((lo + 2048u) >> 12), 0), p.vmax);
        }
      }
    }
    uint32_t x[4], y[4];        /* x = [R, G], y = [B, 0] at output depth: the MHC kernel's packing with C = R, D = B */
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t o[3];
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        if (has_tone) {
          const uint32_t tv = (uint32_t) v[i][ch] << tshift;
          const uint32_t ti = tv >> 8, tf = tv & 255u;
          const uint32_t q = min ((__umul24 (tone[ti], 256u - tf) + __umul24 (tone[ti + 1], tf) + 128u) >> 8, 65535u);
          o[ch] = hp.out16 ? q : q >> 8;
        } else {
          o[ch] = hp.out16 ? (uint32_t) v[i][ch] << s : (uint32_t) v[i][ch] >> s;
        }
      }
      x[i] = o[0] | (o[1] << 16);
      y[i] = o[2];
    }
    uint8_t *out = dst + (size_t) j * (size_t) p.dst_stride;
    const uint32_t s0 = p.sel_cgd[0][0], s1 = p.sel_cgd[0][1];
    if (hp.out16) {
      u32x4 v0, v1;
      emit_cgd<true> (x, y, s0, s1, v0, v1);
      half_store16 (p, out, g, lane, v0, v1);
    } else if (const int planes = p.planar) {
      if (n > 0) {
        const uint32_t col = 4u * (uint32_t) g;
        half_plane (plane_row (p, out, planes & 3) + col, n, gather_byte<0> (x));
        half_plane (plane_row (p, out, (planes >> 2) & 3) + col, n, gather_byte<2> (x));
        half_plane (plane_row (p, out, (planes >> 4) & 3) + col, n, gather_byte<0> (y));
      }
    } else {
      u32x4 vv, unused;
      emit_cgd<false> (x, y, s0, s0, vv, unused);
      half_store8 (out, g, n, p.px3 != 0, vv);
    }
  }
}

hipError_t launch_half (const DeepParams &p, bool in8, bool out16, const ColourStage *stage, int nframes,
    hipStream_t stream)
{
  if (p.width < 1 || p.height < 1 || ((p.px3 || p.planar) && out16) || (p.px3 && p.planar))
    return hipErrorInvalidValue;
  const long long frames = p.nlist > 0 ? p.nlist : nframes;
  if (p.nlist > kMaxList || frames <= 0)
    return frames == 0 ? hipSuccess : hipErrorInvalidValue;
  HalfParams q = {};
  q.d = p;
  q.d.groups = (p.width + kHalfLanePixels - 1) / kHalfLanePixels;
  const int tiles_x = (q.d.groups + 63) / 64;
  const long long chunks_per_frame = (p.height + kHalfRows - 1) / kHalfRows;
  const long long waves = frames * chunks_per_frame * tiles_x;
  if (frames * chunks_per_frame > 0x7fffffffLL || waves > 0x7fffffffLL)
    return hipErrorInvalidValue;
  q.d.div_tiles_x = make_fastdiv ((uint32_t) tiles_x);
  q.d.div_chunks = make_fastdiv ((uint32_t) chunks_per_frame);
  q.d.chunk0 = 0;
  q.d.nwaves = (uint32_t) waves;
  q.in8 = in8;
  q.out16 = out16;
  q.colour = stage != nullptr;
  if (stage)
    q.s = *stage;
  hipLaunchKernelGGL (bayer2rgb_half_kernel, dim3 ((unsigned) ((waves + 3) / 4)), dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* mosaic zone statistics                                                      */
/* ------------------------------------------------------------------------- */
/* Per zone and CFA site: sum and count of the samples in [lo, hi] and the number above hi (include/mibayer.h, group
 * `stats`).  Read-only over the mosaic.  A workgroup is four waves side by side, each on a strip of 64 dwords, walking the
 * (at most kStatsSegRows) rows of one segment of ONE zone row, kStatsAhead dword loads in flight per lane.  A lane's dword
 * holds four 8-bit or two 16-bit samples: two column pairs ("halves") at most, and since a zone is an even number of
 * pixels wide a pair never straddles two zones -- a lane keeps sum / count / clipped per half, column parity and row
 * parity in 32-bit registers (a segment adds at most kStatsSegRows / 2 samples of 16 bits to one of them: no overflow),
 * and adds them once, at the end, into the workgroup's LDS table [zone column][site] with LDS atomics, 64-bit for the
 * sums.  After a barrier the workgroup issues one global atomic per non-zero table entry.  Integer additions: the
 * result does not depend on their order. */
constexpr int kStatsAhead = 8;

__global__ void __launch_bounds__ (256)
mosaic_stats_kernel (StatsParams p)
{
  __shared__ unsigned long long t_sum[kStatsMaxZones * 4];
  __shared__ uint32_t t_cnt[kStatsMaxZones * 4];
  __shared__ uint32_t t_clip[kStatsMaxZones * 4];
  const uint32_t frame = fastdiv (blockIdx.x, p.div_strips);
  const uint32_t strip = blockIdx.x - frame * p.div_strips.d;
  const int zy = (int) blockIdx.y / p.segs;
  const int seg = (int) blockIdx.y - zy * p.segs;
  const int y0 = zy * p.ch + seg * kStatsSegRows;
  int y1 = y0 + kStatsSegRows;
  y1 = y1 < (zy + 1) * p.ch ? y1 : (zy + 1) * p.ch;
  y1 = y1 < p.height ? y1 : p.height;
  if (y0 >= y1)                 /* the whole workgroup: an empty trailing zone row, or a short last segment */
    return;
  t_sum[threadIdx.x] = 0;
  t_cnt[threadIdx.x] = 0;
  t_clip[threadIdx.x] = 0;
  __syncthreads ();

  const int g = (int) (strip * 256u + threadIdx.x);     /* dword of the row */
  if (g < p.row_dwords) {
    const int x0 = p.in8 ? 4 * g : 2 * g;               /* its first column: even, < width */
    const uint32_t w23 = p.in8 && x0 + 2 < p.width ? 1u : 0u;   /* columns x0+2, x0+3 exist */
    const uint8_t *col = p.src + frame * p.src_frame_bytes + 4 * (size_t) g;
    /* [row parity][half][column parity] */
    uint32_t sum[2][2][2] = {}, cnt[2][2][2] = {}, clip[2][2][2] = {};
    /* the samples of dword d, in a row of parity rp; w = 0: the row is past the segment (d = 0) */
    auto add = [&] (uint32_t d, int rp, uint32_t w) {
      uint32_t v[4];
      if (p.in8) {
        v[0] = d & 0xffu;
        v[1] = (d >> 8) & 0xffu;
        v[2] = (d >> 16) & 0xffu;
        v[3] = d >> 24;
      } else {
        const uint32_t m = __builtin_amdgcn_perm (d, d, p.in_sel) & p.mask2;
        v[0] = m & 0xffffu;
        v[1] = m >> 16;
        v[2] = v[3] = 0;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t wk = k < 2 ? w : w & w23;
        const bool in = v[k] - p.lo <= p.hi - p.lo;     /* lo <= v <= hi (lo <= hi) */
        sum[rp][k >> 1][k & 1] += in ? v[k] * wk : 0u;
        cnt[rp][k >> 1][k & 1] += in ? wk : 0u;
        clip[rp][k >> 1][k & 1] += v[k] > p.hi ? wk : 0u;
      }
    };
    int y = y0;                 /* even, and so is kStatsAhead: the row parity below is that of i */
    for (; y + kStatsAhead <= y1; y += kStatsAhead) {
      uint32_t d[kStatsAhead];
#pragma unroll
      for (int i = 0; i < kStatsAhead; i++)
        d[i] = __builtin_nontemporal_load ((const uint32_t *) (col + (size_t) (y + i) * (size_t) p.src_stride));
#pragma unroll
      for (int i = 0; i < kStatsAhead; i++)
        add (d[i], i & 1, 1u);
    }
    for (; y < y1; y += 2) {    /* the last rows of the segment, a pair at a time */
      const bool two = y + 1 < y1;
      const uint32_t d0 = __builtin_nontemporal_load ((const uint32_t *) (col + (size_t) y * (size_t) p.src_stride));
      const uint32_t d1 = two
          ? __builtin_nontemporal_load ((const uint32_t *) (col + (size_t) (y + 1) * (size_t) p.src_stride)) : 0u;
      add (d0, 0, 1u);
      add (d1, 1, two ? 1u : 0u);
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (h == 1 && !w23)
        continue;
      const uint32_t zx = fastdiv ((uint32_t) (x0 + 2 * h), p.div_cw);
#pragma unroll
      for (int site = 0; site < 4; site++) {
        const uint32_t e = zx * 4u + (uint32_t) site;
        const uint32_t n = cnt[site >> 1][h][site & 1], c = clip[site >> 1][h][site & 1];
        if (n) {
          atomicAdd (&t_sum[e], (unsigned long long) sum[site >> 1][h][site & 1]);
          atomicAdd (&t_cnt[e], n);
        }
        if (c)
          atomicAdd (&t_clip[e], c);
      }
    }
  }
  __syncthreads ();
  /* thread t owns table entry t = zone column t / 4, site t % 4 (columns >= zones_x were never added to) */
  const uint32_t e = threadIdx.x;
  unsigned long long *zone = p.stats
      + 8ull * (((unsigned long long) frame * (uint32_t) p.zones_y + (uint32_t) zy) * (uint32_t) p.zones_x + (e >> 2));
  if (t_cnt[e]) {
    atomicAdd (zone + (e & 3u), t_sum[e]);
    atomicAdd ((uint32_t *) (zone + 4) + (e & 3u), t_cnt[e]);
  }
  if (t_clip[e])
    atomicAdd ((uint32_t *) (zone + 6) + (e & 3u), t_clip[e]);
}

hipError_t launch_stats (const StatsParams &p, int nframes, hipStream_t stream)
{
  if (nframes <= 0)
    return nframes == 0 ? hipSuccess : hipErrorInvalidValue;
  if (p.width < 2 || (p.width & 1) || p.height < 1 || p.zones_x < 1 || p.zones_x > kStatsMaxZones || p.zones_y < 1
      || p.ch < 2 || (p.ch & 1) || p.div_cw.d < 2 || (p.div_cw.d & 1)
      || (unsigned long long) p.div_cw.d * (unsigned) p.zones_x < (unsigned) p.width
      || (long long) p.ch * p.zones_y < p.height)
    return hipErrorInvalidValue;        /* (a zone column past the LDS table, a pair across two zones) */
  StatsParams q = p;
  q.row_dwords = p.in8 ? (p.width + 3) / 4 : p.width / 2;
  q.segs = (p.ch + kStatsSegRows - 1) / kStatsSegRows;
  const long long strips = (q.row_dwords + 255) / 256;
  const long long gy = (long long) q.segs * p.zones_y;
  if (strips * nframes > 0x7fffffffLL || gy > 65535)
    return hipErrorInvalidValue;
  q.div_strips = make_fastdiv ((uint32_t) strips);
  hipLaunchKernelGGL (mosaic_stats_kernel, dim3 ((unsigned) (strips * nframes), (unsigned) gy), dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* mosaic histogram                                                            */
/* ------------------------------------------------------------------------- */
/* 256 bins per CFA site over a window of the mosaic (include/mibayer.h, group `hist`).  Read-only over the mosaic.  A
 * workgroup is four waves side by side, each on a strip of 64 dwords, walking seg_rows rows of the window, kHistAhead
 * dword loads in flight per lane.  Every sample is one no-return LDS atomic into the workgroup's table; the table is
 * kept kHistReps times, lane l adding to replica l & 7, so that a wave whose samples all fall into one bin (a flat wall,
 * a clipped sky, a black frame) meets an 8-fold serialisation and not a 64-fold one.  Replica r keeps entry e at
 * r * 1024 + (e ^ 8 r): the eight copies of one entry lie in eight different banks, and a wave reading consecutive
 * entries of one replica reads 64 different banks.  The two samples of a dword that share a site (8-bit mosaic, both
 * column pairs inside) go as one atomic of 2 when they share the bin.  After a barrier thread t sums the replicas of
 * entries t, t + 256, ... and issues one no-return global atomic per non-zero entry: consecutive lanes, consecutive
 * counters.  Integer additions: the result does not depend on their order. */
__global__ void __launch_bounds__ (256)
mosaic_hist_kernel (HistParams p)
{
  __shared__ uint32_t tab[kHistReps * 1024];
  for (int i = (int) threadIdx.x; i < kHistReps * 1024; i += 256)
    tab[i] = 0;
  __syncthreads ();
  const uint32_t frame = fastdiv (blockIdx.x, p.div_strips);
  const uint32_t strip = blockIdx.x - frame * p.div_strips.d;
  const int ya = p.y0 + (int) blockIdx.y * p.seg_rows;  /* < y1 (launch_hist) */
  const int yb = ya + p.seg_rows < p.y1 ? ya + p.seg_rows : p.y1;
  const int g = p.g0 + (int) (strip * 256u + threadIdx.x);      /* dword of the row */
  if (g < p.g1) {
    const int c0 = p.in8 ? 4 * g : 2 * g;               /* its first column: even; a column pair is in or out as a whole */
    const bool in0 = c0 >= p.x0 && c0 < p.x1;
    const bool in1 = p.in8 && c0 + 2 >= p.x0 && c0 + 2 < p.x1;
    const bool both = in0 && in1;
    const uint32_t swz = (threadIdx.x & (kHistReps - 1)) << 3;
    uint32_t *rep = tab + (threadIdx.x & (kHistReps - 1)) * 1024;
    const uint8_t *col = p.src + frame * p.src_frame_bytes + 4 * (size_t) g;
    for (int y = ya; y < yb; y += kHistAhead) {         /* uniform over the workgroup */
      uint32_t d[kHistAhead];
#pragma unroll
      for (int i = 0; i < kHistAhead; i++)
        d[i] = y + i < yb
            ? __builtin_nontemporal_load ((const uint32_t *) (col + (size_t) (y + i) * (size_t) p.src_stride)) : 0u;
#pragma unroll
      for (int i = 0; i < kHistAhead; i++) {
        if (y + i >= yb)
          break;
        const uint32_t sb = (uint32_t) ((y + i) & 1) * 512u;    /* site 2 (y & 1) + column parity */
        uint32_t b0, b1, b2, b3;
        if (p.in8) {
          b0 = d[i] & 0xffu;
          b1 = (d[i] >> 8) & 0xffu;
          b2 = (d[i] >> 16) & 0xffu;
          b3 = d[i] >> 24;
        } else {
          const uint32_t m = __builtin_amdgcn_perm (d[i], d[i], p.in_sel) & p.mask2;
          b0 = b2 = (m & 0xffffu) >> p.shift;
          b1 = b3 = m >> (16 + p.shift);
        }
        const bool e02 = both && b0 == b2, e13 = both && b1 == b3;
        if (in0) {
          atomicAdd (&rep[(sb + b0) ^ swz], e02 ? 2u : 1u);
          atomicAdd (&rep[(sb + 256u + b1) ^ swz], e13 ? 2u : 1u);
        }
        if (in1 && !e02)
          atomicAdd (&rep[(sb + b2) ^ swz], 1u);
        if (in1 && !e13)
          atomicAdd (&rep[(sb + 256u + b3) ^ swz], 1u);
      }
    }
  }
  __syncthreads ();
  uint32_t *out = p.hist + (size_t) frame * 1024u;
  for (uint32_t e = threadIdx.x; e < 1024u; e += 256u) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t r = 0; r < (uint32_t) kHistReps; r++)
      n += tab[r * 1024u + (e ^ (r << 3))];
    if (n)
      atomicAdd (out + e, n);
  }
}

hipError_t launch_hist (const HistParams &p, int nframes, hipStream_t stream)
{
  if (nframes <= 0)
    return nframes == 0 ? hipSuccess : hipErrorInvalidValue;
  if (p.x0 < 0 || (p.x0 & 1) || (p.x1 & 1) || p.x1 < p.x0 + 2 || p.y0 < 0 || p.y1 < p.y0 + 1 || p.shift < 0 || p.shift > 8)
    return hipErrorInvalidValue;        /* (a column pair half inside, a bin past the table) */
  HistParams q = p;
  q.g0 = p.in8 ? p.x0 / 4 : p.x0 / 2;
  q.g1 = p.in8 ? (p.x1 + 3) / 4 : p.x1 / 2;
  const long long strips = (q.g1 - q.g0 + 255) / 256;
  /* Rows per workgroup.  A workgroup merges up to 4 KiB of counters with global atomics and reads seg_rows KiB of mosaic
   * (a strip is 1 KiB wide): at kHistMaxRows the merge is 1/64 of its bytes.  A small launch (one frame on the host path)
   * is cut finer, down to kHistMinRows, until it has kHistSpread workgroups. */
  const long long h = p.y1 - p.y0;
  long long rows = h * strips * nframes / kHistSpread;
  rows = rows < kHistMinRows ? kHistMinRows : rows > kHistMaxRows ? kHistMaxRows : rows;
  if ((h + rows - 1) / rows > 65535)
    rows = (h + 65534) / 65535;
  rows = (rows + 1) & ~1LL;
  const long long gy = (h + rows - 1) / rows;
  if (strips * nframes > 0x7fffffffLL || gy > 65535)
    return hipErrorInvalidValue;
  q.seg_rows = (int) rows;
  q.div_strips = make_fastdiv ((uint32_t) strips);
  hipLaunchKernelGGL (mosaic_hist_kernel, dim3 ((unsigned) (strips * nframes), (unsigned) gy), dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* lens shading correction                                                     */
/* ------------------------------------------------------------------------- */
/* out = clamp (black + (((S - black) G + 2048) >> 12), 0, max) with the gain G interpolated bilinearly, per CFA site,
 * from a grid of Q12 nodes (include/mibayer.h, group `shading`).  Pointwise: a lane reads a dword and writes the same
 * dword, so source and destination may be one mosaic.  A workgroup is four waves side by side, each on a strip of 64
 * dwords, walking seg_rows rows with kShadeAhead dword loads in flight per lane.  A cell is at least 4 pixels wide and
 * starts on a multiple of 4, so the samples of a dword share their cell column: the lane's horizontal weights are fixed,
 * and it keeps, per row parity and sample, the two node rows around the current cell row interpolated horizontally
 * (a[], b[]: at most 32767 * 256 < 2^23).  A row then costs two multiply-adds per sample for G (< 2^31 + rounding, exact
 * in uint32) and one for the sample.  The walk goes cell row by cell row: at a seam -- uniform over the workgroup -- the
 * lower node row becomes the upper one and one new row of nodes is read (2 x 4 gathered 16-bit loads, cached).  Segments
 * and cell rows start on even rows and kShadeAhead is even: the row parity inside the unrolled loop is that of i. */
template <bool IN8>
__global__ void __launch_bounds__ (256)
mosaic_shade_kernel (ShadeParams p)
{
  constexpr int NS = IN8 ? 4 : 2;       /* samples of a dword */
  const uint32_t frame = fastdiv (blockIdx.x, p.div_strips);
  const uint32_t strip = blockIdx.x - frame * p.div_strips.d;
  const int ya = (p.y0 & ~1) + (int) blockIdx.y * p.seg_rows;   /* even; < y1 (launch_shade) */
  const int yb = ya + p.seg_rows < p.y1 ? ya + p.seg_rows : p.y1;
  const int g = (int) (strip * 256u + threadIdx.x);             /* dword of the row */
  if (g >= p.row_dwords)
    return;
  const int x0 = IN8 ? 4 * g : 2 * g;                           /* its first column: even, < width */
  const bool tail = IN8 && x0 + 2 >= p.width;                   /* columns x0 + 2, x0 + 3 are past the row's end */
  const bool in_place = (const uint8_t *) p.dst == p.src;
  const uint32_t cw = 1u << p.kx, ch = 1u << p.ky;
  const int sh = p.kx + p.ky;
  const uint32_t rnd = 1u << (sh - 1);
  uint32_t wl[NS], wr[NS];
#pragma unroll
  for (int k = 0; k < NS; k++) {
    wr[k] = (uint32_t) (x0 + k) & (cw - 1u);
    wl[k] = cw - wr[k];
  }
  /* node row jr of the four site planes, at the lane's cell column and the one right of it (ci + 1 <= nx - 1) */
  const uint16_t *tab = p.table + (x0 >> p.kx);
  auto node_row = [&] (int jr, uint32_t (&h)[2][NS]) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const uint16_t *n = tab + ((size_t) s * (size_t) p.ny + (size_t) jr) * (size_t) p.nx;
      const uint32_t l = n[0], r = n[1];
#pragma unroll
      for (int k = s & 1; k < NS; k += 2)
        h[s >> 1][k] = l * wl[k] + r * wr[k];
    }
  };
  const uint8_t *scol = p.src + frame * p.src_frame_bytes + 4 * (size_t) g;
  uint8_t *dcol = p.dst + frame * p.dst_frame_bytes + 4 * (size_t) g;
  int j = ya >> p.ky;                   /* j + 1 <= ny - 1 (launch_shade) */
  uint32_t a[2][NS], b[2][NS];
  node_row (j, a);
  node_row (j + 1, b);
  for (int y = ya; y < yb;) {           /* uniform over the workgroup; y is even here */
    if ((y >> p.ky) != j) {             /* a cell-row seam */
      j = y >> p.ky;
#pragma unroll
      for (int k = 0; k < NS; k++) {
        a[0][k] = b[0][k];
        a[1][k] = b[1][k];
      }
      node_row (j + 1, b);
    }
    const int seam = (j + 1) << p.ky;
    const int ye = seam < yb ? seam : yb;
    for (int yy = y; yy < ye; yy += kShadeAhead) {
      const uint32_t fy0 = (uint32_t) yy & (ch - 1u);
      uint32_t d[kShadeAhead];
#pragma unroll
      for (int i = 0; i < kShadeAhead; i++)
        d[i] = yy + i < ye
            ? __builtin_nontemporal_load ((const uint32_t *) (scol + (size_t) (yy + i) * (size_t) p.src_stride)) : 0u;
#pragma unroll
      for (int i = 0; i < kShadeAhead; i++) {
        if (yy + i >= ye)
          break;
        if (yy + i < p.y0)              /* the row under an odd y0 */
          continue;
        const uint32_t fy = fy0 + (uint32_t) i;         /* < ch: the rows up to ye lie in cell row j */
        uint32_t v[NS];
        if (IN8) {
#pragma unroll
          for (int k = 0; k < NS; k++)
            v[k] = (d[i] >> (8 * k)) & 0xffu;
        } else {
          const uint32_t m = __builtin_amdgcn_perm (d[i], d[i], p.in_sel) & p.mask2;
          v[0] = m & 0xffffu;
          v[NS - 1] = m >> 16;
        }
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < NS; k++) {
          const uint32_t gain = (a[i & 1][k] * (ch - fy) + b[i & 1][k] * fy + rnd) >> sh;       /* <= 32767 */
          const int bl = p.black[2 * (i & 1) + (k & 1)];
          int q = bl + ((((int) v[k] - bl) * (int) gain + 2048) >> 12);
          q = q < 0 ? 0 : q > p.vmax ? p.vmax : q;
          o |= (uint32_t) q << ((IN8 ? 8 : 16) * k);
        }
        if (!IN8)
          o = __builtin_amdgcn_perm (o, o, p.in_sel);
        uint8_t *out = dcol + (size_t) (yy + i) * (size_t) p.dst_stride;
        if (tail)
          *(uint16_t *) out = (uint16_t) o;
        else if (in_place)
          *(uint32_t *) out = o;
        else
          __builtin_nontemporal_store (o, (uint32_t *) out);
      }
    }
    y = ye;
  }
}

hipError_t launch_shade (const ShadeParams &p, int nframes, hipStream_t stream)
{
  if (nframes <= 0)
    return nframes == 0 ? hipSuccess : hipErrorInvalidValue;
  if (p.width < 2 || (p.width & 1) || p.kx < 2 || p.kx > 8 || p.ky < 2 || p.ky > 8 || p.y0 < 0 || p.y1 <= p.y0
      || p.y1 > p.height || p.nx < ((p.width - 1) >> p.kx) + 2 || p.ny < ((p.height - 1) >> p.ky) + 2 || !p.table)
    return hipErrorInvalidValue;        /* (a node past the table, a cell narrower than a dword) */
  ShadeParams q = p;
  q.row_dwords = p.in8 ? (p.width + 3) / 4 : p.width / 2;
  const long long strips = (q.row_dwords + 255) / 256;
  /* rows per workgroup: as many as kShadeMaxRows, cut finer (one frame on the host path, one band of it) until the
   * launch has kShadeSpread workgroups */
  const long long h = p.y1 - (p.y0 & ~1);
  long long rows = h * strips * nframes / kShadeSpread;
  rows = rows < kShadeMinRows ? kShadeMinRows : rows > kShadeMaxRows ? kShadeMaxRows : rows;
  if ((h + rows - 1) / rows > 65535)
    rows = (h + 65534) / 65535;
  rows = (rows + 1) & ~1LL;
  const long long gy = (h + rows - 1) / rows;
  if (strips * nframes > 0x7fffffffLL || gy > 65535)
    return hipErrorInvalidValue;
  q.seg_rows = (int) rows;
  q.div_strips = make_fastdiv ((uint32_t) strips);
  const dim3 grid ((unsigned) (strips * nframes), (unsigned) gy);
  if (p.in8)
    hipLaunchKernelGGL (mosaic_shade_kernel<true>, grid, dim3 (256), 0, stream, q);
  else
    hipLaunchKernelGGL (mosaic_shade_kernel<false>, grid, dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* defective pixel correction                                                  */
/* ------------------------------------------------------------------------- */
/* out = R where S > hi + hot or S + cold < lo, else S, over the eight same-site neighbours at +-2 (include/mibayer.h,
 * group `dpc`).  All of it is done on dwords that hold two samples in their 16-bit halves: the two words of a deep
 * mosaic, or the even and the odd bytes of an 8-bit dword, so one body serves both widths and the 8-bit kernel calls it
 * twice.  No value leaves its half: every sample is at most 0xffff, the differences saturate, and
 * R = (a + b + 1) >> 1 = (a | b) - ((a ^ b) >> 1) borrows nothing. */
typedef unsigned short dpc_u16x2 __attribute__ ((ext_vector_type (2)));
#define DPC_V(x) __builtin_bit_cast (dpc_u16x2, (uint32_t) (x))
#define DPC_U(v) __builtin_bit_cast (uint32_t, (v))
__device__ __forceinline__ uint32_t dpc_max (uint32_t a, uint32_t b) { return DPC_U (__builtin_elementwise_max (DPC_V (a), DPC_V (b))); }
__device__ __forceinline__ uint32_t dpc_min (uint32_t a, uint32_t b) { return DPC_U (__builtin_elementwise_min (DPC_V (a), DPC_V (b))); }
/* max (a - b, 0) per half */
__device__ __forceinline__ uint32_t dpc_over (uint32_t a, uint32_t b) { return DPC_U (__builtin_elementwise_sub_sat (DPC_V (a), DPC_V (b))); }
/* 0xffff in the halves that are not zero: 0 - min (a, 1), two packed instructions.  `one` is 1 in both halves from a
 * register the compiler cannot see into (mosaic_dpc_kernel): knowing the constant it turns the minimum into a compare and
 * a select per half and puts the halves together again, seven instructions */
__device__ __forceinline__ uint32_t dpc_any (uint32_t a, uint32_t one)
{
  return DPC_U (DPC_V (0u) - DPC_V (dpc_min (a, one)));
}

/* the pair (a, b) replaces the best pair so far where its gradient is smaller; the first of equals stays */
__device__ __forceinline__ void dpc_pair (uint32_t a, uint32_t b, uint32_t &bg, uint32_t &ba, uint32_t &bb, uint32_t one)
{
  const uint32_t g = dpc_max (a, b) - dpc_min (a, b);
  const uint32_t m = dpc_any (dpc_over (bg, g), one);
  bg = dpc_min (bg, g);
  ba = (a & m) | (ba & ~m);
  bb = (b & m) | (bb & ~m);
}

/* rows up / mid / down of the window as (left, centre, right): the samples two columns left of, at and two columns right
 * of the lane's; hot, cold: the thresholds in both halves, 0xffff = never */
__device__ __forceinline__ uint32_t dpc_samples (const uint32_t *u, const uint32_t *m, const uint32_t *d, uint32_t hot, uint32_t cold,
    uint32_t one)
{
  const uint32_t s = m[1];
  const uint32_t hi = dpc_max (dpc_max (dpc_max (u[0], u[1]), dpc_max (u[2], m[0])),
      dpc_max (dpc_max (m[2], d[0]), dpc_max (d[1], d[2])));
  const uint32_t lo = dpc_min (dpc_min (dpc_min (u[0], u[1]), dpc_min (u[2], m[0])),
      dpc_min (dpc_min (m[2], d[0]), dpc_min (d[1], d[2])));
  const uint32_t bad = dpc_any (dpc_over (dpc_over (s, hi), hot) | dpc_over (dpc_over (lo, s), cold), one);
  uint32_t ba = m[0], bb = m[2];                                                /* H */
  uint32_t bg = dpc_max (ba, bb) - dpc_min (ba, bb);
  dpc_pair (u[1], d[1], bg, ba, bb, one);                                            /* V */
  dpc_pair (u[0], d[2], bg, ba, bb, one);                                            /* D1 */
  dpc_pair (u[2], d[0], bg, ba, bb, one);                                            /* D2 */
  const uint32_t r = (ba | bb) - (((ba ^ bb) >> 1) & 0x7fff7fffu);
  return (r & bad) | (s & ~bad);
}

/* The detection and copy pass.  A workgroup is four waves side by side, each on a strip of 64 dwords, walking seg_rows
 * rows; a lane owns a dword column and holds a rolling window of five rows plus the one in flight, each as the dwords
 * left of, at and right of its own (three coalesced loads per row; the neighbours' come from the cache), so a row is
 * fetched once per segment plus four halo rows.  The row three below is requested before the current row is computed and
 * unpacked after it: a load has a whole row of arithmetic to arrive in.  The borders are substituted at load time: the
 * row index is mirrored around the pixel (t - 2 < 0 -> t + 2 is row t + 4 of the loaded one) and the dword off the row's
 * end is replaced by the one on the other side.  Of an 8-bit mosaic the samples two columns away are the two halves of a
 * byte-aligned pair of dwords, and a row is kept as its even and its odd bytes (NP = 2 dwords of packed halves per
 * position); a row whose width is 2 mod 4 ends in half a dword, which takes its right-hand neighbours from its upper
 * half and is stored as 16 bits. */
template <bool IN8>
__global__ void __launch_bounds__ (256)
mosaic_dpc_kernel (DpcParams p)
{
  constexpr int NP = IN8 ? 2 : 1;
  const uint32_t frame = fastdiv (blockIdx.x, p.div_strips);
  const uint32_t strip = blockIdx.x - frame * p.div_strips.d;
  const int ya = p.y0 + (int) blockIdx.y * p.seg_rows;          /* < y1 (launch_dpc) */
  const int yb = ya + p.seg_rows < p.y1 ? ya + p.seg_rows : p.y1;
  const int g = (int) (strip * 256u + threadIdx.x);             /* dword of the row */
  if (g >= p.row_dwords)
    return;
  const int last = p.row_dwords - 1;
  const bool tail = IN8 && 4 * g + 2 >= p.width;                /* columns 4 g + 2, 4 g + 3 are past the row's end */
  const int gl = g > 0 ? g - 1 : IN8 ? g : g + 1;               /* 0 .. last, as is gr */
  const int gr = g < last ? g + 1 : IN8 ? g : g - 1;
  const uint32_t hot = p.hot < 0 ? 0xffffffffu : (uint32_t) p.hot * 0x10001u;
  const uint32_t cold = p.cold < 0 ? 0xffffffffu : (uint32_t) p.cold * 0x10001u;
  uint32_t one = 0x00010001u;
  asm ("" : "+v" (one));        /* dpc_any */
  const uint8_t *sbase = p.src + frame * p.src_frame_bytes;
  uint8_t *dcol = p.dst + frame * p.dst_frame_bytes + 4 * (size_t) g;
  /* row t of the window, -2 <= t < height + 2: rows 0 .. height - 1 of the source only (height >= 4); past the
   * segment's own halo nothing is needed, and the last row asked for is loaded again */
  auto load_row = [&] (int t, uint32_t (&raw)[3]) {
    t = t < yb + 1 ? t : yb + 1;
    const int r = t < 0 ? t + 4 : t >= p.height ? t - 4 : t;
    const uint32_t *row = (const uint32_t *) (sbase + (size_t) r * (size_t) p.src_stride);
    raw[0] = row[gl];
    raw[1] = row[g];
    raw[2] = row[gr];
  };
  /* the loaded dwords as (left, centre, right) of packed halves: w[j * NP + k] */
  auto unpack_row = [&] (const uint32_t (&raw)[3], uint32_t (&w)[3 * NP]) {
    if (IN8) {
      const uint32_t b = tail ? (raw[1] & 0xffffu) | (raw[0] & 0xffff0000u) : raw[1];
      const uint32_t t[3] = { __builtin_amdgcn_alignbyte (b, raw[0], 2), b, __builtin_amdgcn_alignbyte (raw[2], b, 2) };
#pragma unroll
      for (int j = 0; j < 3; j++) {
        w[j * NP] = t[j] & 0x00ff00ffu;
        w[j * NP + NP - 1] = (t[j] >> 8) & 0x00ff00ffu;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 3; j++)
        w[j * NP] = __builtin_amdgcn_perm (raw[j], raw[j], p.in_sel) & p.mask2;
    }
  };
  uint32_t w[5][3 * NP], raw[3];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    load_row (ya - 2 + k, raw);
    unpack_row (raw, w[k]);
  }
  for (int y = ya; y < yb; y++) {       /* uniform over the workgroup */
    load_row (y + 3, raw);
    uint32_t o;
    if (IN8) {
      const uint32_t ue[3] = { w[0][0], w[0][2], w[0][4] }, me[3] = { w[2][0], w[2][2], w[2][4] }, de[3] = { w[4][0], w[4][2], w[4][4] };
      const uint32_t uo[3] = { w[0][1], w[0][3], w[0][5] }, mo[3] = { w[2][1], w[2][3], w[2][5] }, dq[3] = { w[4][1], w[4][3], w[4][5] };
      o = dpc_samples (ue, me, de, hot, cold, one) | (dpc_samples (uo, mo, dq, hot, cold, one) << 8);
    } else {
      o = dpc_samples (w[0], w[2], w[4], hot, cold, one);
      o = __builtin_amdgcn_perm (o, o, p.in_sel);
    }
    uint8_t *out = dcol + (size_t) y * (size_t) p.dst_stride;
    if (tail)
      *(uint16_t *) out = (uint16_t) o;
    else
      __builtin_nontemporal_store (o, (uint32_t *) out);
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int j = 0; j < 3 * NP; j++)
        w[k][j] = w[k + 1][j];
    unpack_row (raw, w[4]);
  }
}

/* The listed defects of rows [y0, y1): one lane per entry [list_lo, list_hi) and frame, behind the pass above on the
 * same stream.  R is computed from the source, so an entry the detection has flagged too receives the same value. */
__global__ void __launch_bounds__ (256)
mosaic_dpc_list_kernel (DpcParams p)
{
  const uint32_t per = ((uint32_t) (p.list_hi - p.list_lo) + 255u) / 256u;     /* workgroups per frame */
  const uint32_t frame = blockIdx.x / per;
  const int e = p.list_lo + (int) ((blockIdx.x - frame * per) * 256u + threadIdx.x);
  if (e >= p.list_hi)
    return;
  const int x = (int) p.list[2 * e], y = (int) p.list[2 * e + 1];       /* inside the frame (mibayer_set_dpc) */
  const int xl = x >= 2 ? x - 2 : x + 2, xr = x + 2 < p.width ? x + 2 : x - 2;
  const int yu = y >= 2 ? y - 2 : y + 2, yd = y + 2 < p.height ? y + 2 : y - 2;
  const uint8_t *src = p.src + frame * p.src_frame_bytes;
  auto at = [&] (int xx, int yy) -> int {
    const uint8_t *row = src + (size_t) yy * (size_t) p.src_stride;
    if (p.in8)
      return row[xx];
    const uint32_t v = ((const uint16_t *) row)[xx];
    return (int) (__builtin_amdgcn_perm (v, v, p.in_sel) & p.mask2 & 0xffffu);
  };
  const int pa[4] = { at (xl, y), at (x, yu), at (xl, yu), at (xr, yu) };
  const int pb[4] = { at (xr, y), at (x, yd), at (xr, yd), at (xl, yd) };
  int bg = 0x10000, r = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int gk = pa[k] > pb[k] ? pa[k] - pb[k] : pb[k] - pa[k];
    if (gk < bg) {
      bg = gk;
      r = (pa[k] + pb[k] + 1) >> 1;
    }
  }
  uint8_t *out = p.dst + frame * p.dst_frame_bytes + (size_t) y * (size_t) p.dst_stride;
  if (p.in8)
    out[x] = (uint8_t) r;
  else
    ((uint16_t *) out)[x] = (uint16_t) __builtin_amdgcn_perm ((uint32_t) r, (uint32_t) r, p.in_sel);
}

hipError_t launch_dpc (const DpcParams &p, int nframes, hipStream_t stream)
{
  if (nframes <= 0)
    return nframes == 0 ? hipSuccess : hipErrorInvalidValue;
  if (p.width < 4 || (p.width & 1) || p.height < 4 || p.y0 < 0 || p.y1 <= p.y0 || p.y1 > p.height || p.dst == p.src
      || p.list_lo < 0 || p.list_hi < p.list_lo || (p.list_hi > p.list_lo && !p.list))
    return hipErrorInvalidValue;        /* (a mirrored row or dword outside the frame) */
  DpcParams q = p;
  q.row_dwords = p.in8 ? (p.width + 3) / 4 : p.width / 2;
  const long long strips = (q.row_dwords + 255) / 256;
  /* rows per workgroup as in launch_shade: as many as kDpcMaxRows, cut finer until the launch has kDpcSpread workgroups */
  const long long h = p.y1 - p.y0;
  long long rows = h * strips * nframes / kDpcSpread;
  rows = rows < kDpcMinRows ? kDpcMinRows : rows > kDpcMaxRows ? kDpcMaxRows : rows;
  if ((h + rows - 1) / rows > 65535)
    rows = (h + 65534) / 65535;
  const long long gy = (h + rows - 1) / rows;
  const long long per = ((long long) (p.list_hi - p.list_lo) + 255) / 256;
  if (strips * nframes > 0x7fffffffLL || gy > 65535 || per * nframes > 0x7fffffffLL)
    return hipErrorInvalidValue;
  q.seg_rows = (int) rows;
  q.div_strips = make_fastdiv ((uint32_t) strips);
  const dim3 grid ((unsigned) (strips * nframes), (unsigned) gy);
  if (p.in8)
    hipLaunchKernelGGL (mosaic_dpc_kernel<true>, grid, dim3 (256), 0, stream, q);
  else
    hipLaunchKernelGGL (mosaic_dpc_kernel<false>, grid, dim3 (256), 0, stream, q);
  if (per > 0)
    hipLaunchKernelGGL (mosaic_dpc_list_kernel, dim3 ((unsigned) (per * nframes)), dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* noise reduction                                                             */
/* ------------------------------------------------------------------------- */
/* out = the rounded mean of S and those of its 24 same-site neighbours at +-2 and +-4 that lie within t (S) of it
 * (include/mibayer.h, group `nr`).  As in the defect pass everything up to the division is done on dwords that hold two
 * samples in their 16-bit halves, so one body serves both widths and the 8-bit kernel calls it twice: the differences
 * saturate, the weight is 0 or 1, and P, N <= 24 * 2047 and cnt <= 25 stay in their halves. */

/* neighbours n against centres s: where |n - s| <= t (t1 = t + 1 per half) n - s goes to P or s - n to N, and cnt counts */
__device__ __forceinline__ void nr_tap (uint32_t n, uint32_t s, uint32_t t1, uint32_t one, uint32_t &P, uint32_t &N, uint32_t &cnt)
{
  const uint32_t dp = dpc_over (n, s), dn = dpc_over (s, n);            /* one of the two is 0 */
  const uint32_t w = dpc_min (dpc_over (t1, dp | dn), one);
  P = DPC_U (DPC_V (w) * DPC_V (dp) + DPC_V (P));
  N = DPC_U (DPC_V (w) * DPC_V (dn) + DPC_V (N));
  cnt = DPC_U (DPC_V (cnt) + DPC_V (w));
}

/* t + 1 of one sample: the curve between its nodes k and k + 1 (lut[k] = curve[k], curve[k + 1] - curve[k]), which is
 * (curve[k] (s - f) + curve[k + 1] f + s / 2) >> sh since curve[k] s is a multiple of s and >> floors */
__device__ __forceinline__ uint32_t nr_threshold (uint32_t s, const int2 *lut, int sh)
{
  const int2 c = lut[s >> sh];
  const int f = (int) (s & ((1u << sh) - 1u));
  return (uint32_t) (c.x + ((c.y * f + (1 << (sh - 1))) >> sh)) + 1u;
}

/* out of one sample: S +- (2 |v| + cnt) / (2 cnt), v = P - N, by the reciprocal (tests/test_nr_model.py proves it exact) */
__device__ __forceinline__ uint32_t nr_mean (uint32_t s, uint32_t P, uint32_t N, uint32_t cnt, const uint32_t *rcp)
{
  const int v = (int) P - (int) N;
  const uint32_t a = (uint32_t) (v < 0 ? -v : v);
  const uint32_t q = __umulhi (2u * a + cnt, rcp[cnt]);
  return v < 0 ? s - q : s + q;
}

/* r[0 .. 4]: the rows at -4, -2, 0, 2, 4, each as the five dwords of packed halves at -4, -2, 0, 2, 4 columns */
__device__ __forceinline__ uint32_t nr_samples (const uint32_t (&r)[5][5], const int2 *lut, const uint32_t *rcp, int sh, uint32_t one)
{
  const uint32_t s = r[2][2];
  const uint32_t t1 = nr_threshold (s & 0xffffu, lut, sh) | (nr_threshold (s >> 16, lut, sh) << 16);
  uint32_t P = 0, N = 0, cnt = 0x00010001u;
#pragma unroll
  for (int k = 0; k < 5; k++)
#pragma unroll
    for (int j = 0; j < 5; j++)
      if (k != 2 || j != 2)
        nr_tap (r[k][j], s, t1, one, P, N, cnt);
  return nr_mean (s & 0xffffu, P & 0xffffu, N & 0xffffu, cnt & 0xffffu, rcp)
      | (nr_mean (s >> 16, P >> 16, N >> 16, cnt >> 16, rcp) << 16);
}

/* The geometry is mosaic_dpc_kernel's: four waves side by side, a lane per dword column, seg_rows rows per workgroup, and
 * a rolling window in registers, here of nine rows, of which a row uses every other one.  A row of the window is kept as
 * its five tap dwords -- the samples at -4, -2, 0, +2, +4 columns of the lane's: for a deep mosaic the dwords at -2 .. +2,
 * unpacked; for an 8-bit one the dwords at -1, 0, +1 and the two byte-aligned pairs between them, still as bytes, split
 * into even and odd bytes when used (45 registers; the 90 of the unpacked halves would not leave four waves per SIMD).
 * The row five below is requested before the current row is computed and turned into taps after it.
 * The borders are substituted at load time.  Rows: the index is reflected about the edge row.  Columns: the lanes at a
 * row's ends load the dwords inside the row that hold the reflected samples (the dword index reflected likewise; in an
 * 8-bit row the first lane's left dword is its right one and the last lane's right dword its left one) and a v_perm per
 * tap, whose selector is the identity in every other lane, puts the reflected samples in place.  A row of an 8-bit mosaic
 * whose width is 2 mod 4 ends in half a dword: that lane continues its dword with the reflected samples, computes four
 * and stores two. */
template <bool IN8>
__global__ void __launch_bounds__ (256)
mosaic_nr_kernel (NrParams p)
{
  constexpr int NRAW = IN8 ? 3 : 5;
  __shared__ int2 lut[16];
  __shared__ uint32_t rcp[32];
  if (threadIdx.x < 16)
    lut[threadIdx.x] = make_int2 (p.lut[threadIdx.x][0], p.lut[threadIdx.x][1]);
  else if (threadIdx.x >= 32 && threadIdx.x < 58)
    rcp[threadIdx.x - 32] = p.rcp[threadIdx.x - 32];
  __syncthreads ();
  const uint32_t frame = fastdiv (blockIdx.x, p.div_strips);
  const uint32_t strip = blockIdx.x - frame * p.div_strips.d;
  const int ya = p.y0 + (int) blockIdx.y * p.seg_rows;          /* < y1 (launch_nr) */
  const int yb = ya + p.seg_rows < p.y1 ? ya + p.seg_rows : p.y1;
  const int g = (int) (strip * 256u + threadIdx.x);             /* dword of the row */
  if (g >= p.row_dwords)
    return;
  const int last = p.row_dwords - 1;                            /* >= 1 (8-bit), >= 2 (deep) */
  const bool tail = IN8 && 4 * g + 2 >= p.width;                /* columns 4 g + 2, 4 g + 3 are past the row's end */
  uint32_t one = 0x00010001u;
  asm ("" : "+v" (one));        /* dpc_any */
  int idx[NRAW];                /* the dwords loaded, all of them 0 .. last */
  uint32_t sel[NRAW];           /* the selectors that turn them into taps */
  constexpr uint32_t kFirst = 0x07060504u;      /* v_perm (a, b, sel): a */
  if constexpr (IN8) {
    idx[0] = g > 0 ? g - 1 : g + 1;
    idx[1] = g;
    idx[2] = g < last ? g + 1 : g - 1;
    /* columns -4 .. -1 are columns 4, 3, 2, 1: (a, b) = (dword 1, dword 0) */
    sel[0] = g > 0 ? kFirst : 0x01020304u;
    /* the half dword goes on with columns W - 2, W - 3: (a, b) = (itself, the dword left of it) */
    sel[1] = tail ? 0x03040504u : kFirst;
    /* (a, b) = (dword idx[2], the lane's own).  The last dword, whole: columns W .. W + 3 are W - 2 .. W - 5; the half
     * one: W + 2, W + 3 are W - 4, W - 5 of the dword left of it; the one left of the half one: W - 2, W - 1, W - 2, W - 3 */
    sel[2] = g == last ? (tail ? 0x07060506u : 0x07000102u) : (g == last - 1 && (p.width & 2)) ? 0x03040504u : kFirst;
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const int d = g + k - 2;
      idx[k] = d < 0 ? -d : d > last ? 2 * last - d : d;
    }
    /* a dword off the left end is (low half of its reflection, high half of the dword right of that), one off the right
     * end (low half of the dword left of its reflection, high half of the reflection); taps 0, 1, 3, 4 are
     * v_perm (dword k, its neighbour towards the centre), then comes the byte order */
    const uint32_t left = 0x03020504u, right = 0x07060100u;
    const uint32_t base[5] = { g < 2 ? left : kFirst, g < 1 ? left : kFirst, kFirst, g + 1 > last ? right : kFirst,
      g + 2 > last ? right : kFirst };
#pragma unroll
    for (int k = 0; k < 5; k++)
      sel[k] = __builtin_amdgcn_perm (base[k], base[k], p.in_sel);
  }
  const uint8_t *sbase = p.src + frame * p.src_frame_bytes;
  uint8_t *dcol = p.dst + frame * p.dst_frame_bytes + 4 * (size_t) g;
  /* row t of the window, -4 <= t < height + 4: rows 0 .. height - 1 of the source only (height >= 5); past the segment's
   * own halo nothing is needed, and the last row asked for is loaded again */
  auto load_row = [&] (int t, uint32_t (&raw)[NRAW]) {
    t = t < yb + 3 ? t : yb + 3;
    const int r = t < 0 ? -t : t >= p.height ? 2 * (p.height - 1) - t : t;
    const uint32_t *row = (const uint32_t *) (sbase + (size_t) r * (size_t) p.src_stride);
#pragma unroll
    for (int k = 0; k < NRAW; k++)
      raw[k] = row[idx[k]];
  };
  auto taps_of = [&] (const uint32_t (&raw)[NRAW], uint32_t (&w)[5]) {
    if constexpr (IN8) {
      const uint32_t c = __builtin_amdgcn_perm (raw[1], raw[0], sel[1]);
      w[0] = __builtin_amdgcn_perm (raw[0], raw[1], sel[0]);
      w[4] = __builtin_amdgcn_perm (raw[2], raw[1], sel[2]);
      w[1] = __builtin_amdgcn_alignbyte (c, w[0], 2);
      w[2] = c;
      w[3] = __builtin_amdgcn_alignbyte (w[4], c, 2);
    } else {
      w[0] = __builtin_amdgcn_perm (raw[0], raw[1], sel[0]) & p.mask2;
      w[1] = __builtin_amdgcn_perm (raw[1], raw[2], sel[1]) & p.mask2;
      w[2] = __builtin_amdgcn_perm (raw[2], raw[2], sel[2]) & p.mask2;
      w[3] = __builtin_amdgcn_perm (raw[3], raw[2], sel[3]) & p.mask2;
      w[4] = __builtin_amdgcn_perm (raw[4], raw[3], sel[4]) & p.mask2;
    }
  };
  uint32_t w[9][5], raw[NRAW];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    load_row (ya - 4 + k, raw);
    taps_of (raw, w[k]);
  }
  for (int y = ya; y < yb; y++) {       /* uniform over the workgroup */
    load_row (y + 5, raw);
    uint32_t o;
    if (IN8) {
      uint32_t h[5][5];
#pragma unroll
      for (int k = 0; k < 5; k++)
#pragma unroll
        for (int j = 0; j < 5; j++)
          h[k][j] = w[2 * k][j] & 0x00ff00ffu;
      o = nr_samples (h, lut, rcp, p.shift, one);
#pragma unroll
      for (int k = 0; k < 5; k++)
#pragma unroll
        for (int j = 0; j < 5; j++)
          h[k][j] = (w[2 * k][j] >> 8) & 0x00ff00ffu;
      o |= nr_samples (h, lut, rcp, p.shift, one) << 8;
    } else {
      const uint32_t h[5][5] = { { w[0][0], w[0][1], w[0][2], w[0][3], w[0][4] }, { w[2][0], w[2][1], w[2][2], w[2][3], w[2][4] },
        { w[4][0], w[4][1], w[4][2], w[4][3], w[4][4] }, { w[6][0], w[6][1], w[6][2], w[6][3], w[6][4] },
        { w[8][0], w[8][1], w[8][2], w[8][3], w[8][4] } };
      o = nr_samples (h, lut, rcp, p.shift, one);
      o = __builtin_amdgcn_perm (o, o, p.in_sel);
    }
    uint8_t *out = dcol + (size_t) y * (size_t) p.dst_stride;
    if (tail)
      *(uint16_t *) out = (uint16_t) o;
    else
      __builtin_nontemporal_store (o, (uint32_t *) out);
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
      for (int j = 0; j < 5; j++)
        w[k][j] = w[k + 1][j];
    taps_of (raw, w[8]);
  }
}

hipError_t launch_nr (const NrParams &p, int nframes, hipStream_t stream)
{
  if (nframes <= 0)
    return nframes == 0 ? hipSuccess : hipErrorInvalidValue;
  if (p.width < 6 || (p.width & 1) || p.height < 5 || p.y0 < 0 || p.y1 <= p.y0 || p.y1 > p.height || p.dst == p.src
      || p.shift < 4 || p.shift > 12)
    return hipErrorInvalidValue;        /* (a reflected row or dword outside the frame) */
  NrParams q = p;
  q.rcp[0] = 0;
  for (uint32_t cnt = 1; cnt <= 25; cnt++)
    q.rcp[cnt] = (uint32_t) (((1ull << 32) + 2 * cnt - 1) / (2 * cnt));
  q.row_dwords = p.in8 ? (p.width + 3) / 4 : p.width / 2;
  const long long strips = (q.row_dwords + 255) / 256;
  /* rows per workgroup as in launch_dpc */
  const long long h = p.y1 - p.y0;
  long long rows = h * strips * nframes / kNrSpread;
  rows = rows < kNrMinRows ? kNrMinRows : rows > kNrMaxRows ? kNrMaxRows : rows;
  if ((h + rows - 1) / rows > 65535)
    rows = (h + 65534) / 65535;
  const long long gy = (h + rows - 1) / rows;
  if (strips * nframes > 0x7fffffffLL || gy > 65535)
    return hipErrorInvalidValue;
  q.seg_rows = (int) rows;
  q.div_strips = make_fastdiv ((uint32_t) strips);
  const dim3 grid ((unsigned) (strips * nframes), (unsigned) gy);
  if (p.in8)
    hipLaunchKernelGGL (mosaic_nr_kernel<true>, grid, dim3 (256), 0, stream, q);
  else
    hipLaunchKernelGGL (mosaic_nr_kernel<false>, grid, dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* mosaic focus statistics                                                     */
/* ------------------------------------------------------------------------- */
/* Per zone and CFA site: sum and number of the same-site second differences |2 S - S(-2) - S(+2)|, across and down, that
 * reach the threshold (include/mibayer.h, group `focus`).  Read-only over the mosaic.  The launch geometry is
 * mosaic_stats_kernel's -- four waves side by side, a lane per dword column, one segment of at most kStatsSegRows rows of
 * ONE zone row per workgroup -- and the stencil is mosaic_dpc_kernel's: a rolling window of the lane's own dword of five
 * rows, y - 2 .. y + 2, the row three below requested before the current one is computed.  A row arrives as the dwords
 * left of, at and right of the lane's (three coalesced loads; the neighbours' come from the cache); its horizontal
 * responses are taken as it arrives and only its own dword enters the window, its vertical ones when it is the window's
 * middle.  Nothing is substituted at a border: a row index outside the frame and a dword off the row's end are clamped
 * for the address only, and what does not exist is masked -- `hmask` / `vmask` per 16-bit half of the lane, and `own` /
 * `vok` per row, uniform over the workgroup.  Rows of another frame are never addressed.
 * Of a deep mosaic the two samples of a dword are computed in 32 bits (|r| <= 2 * 65535).  Of an 8-bit mosaic a row is
 * kept as its even and its odd bytes, two samples in the 16-bit halves of a dword as in mosaic_dpc_kernel: |r| <= 510 and
 * at most kStatsSegRows / 2 rows of one parity fall in a segment, so a half holds the arithmetic (no value leaves its
 * half: a + b and 2 c are at most 510, max - min borrows nothing) and the sums (32 * 510 < 65536).  The low half is the
 * lane's first column pair, the high half its second; a pair never straddles two zones.  A lane keeps sum and count per
 * row parity, column parity (and half) in registers and adds them once into the workgroup's LDS table
 * [zone column][site], 64-bit for the sums; after a barrier the workgroup issues one global atomic per non-zero entry.
 * Integer additions: the result does not depend on their order. */
template <bool IN8>
__global__ void __launch_bounds__ (256)
mosaic_focus_kernel (FocusParams p)
{
  constexpr int NP = IN8 ? 2 : 1;
  __shared__ unsigned long long t_h[kStatsMaxZones * 4];
  __shared__ unsigned long long t_v[kStatsMaxZones * 4];
  __shared__ uint32_t t_nh[kStatsMaxZones * 4];
  __shared__ uint32_t t_nv[kStatsMaxZones * 4];
  const uint32_t frame = fastdiv (blockIdx.x, p.div_strips);
  const uint32_t strip = blockIdx.x - frame * p.div_strips.d;
  const int zy = (int) blockIdx.y / p.segs;
  const int seg = (int) blockIdx.y - zy * p.segs;
  const int y0 = zy * p.ch + seg * kStatsSegRows;       /* even */
  int y1 = y0 + kStatsSegRows;
  y1 = y1 < (zy + 1) * p.ch ? y1 : (zy + 1) * p.ch;
  y1 = y1 < p.height ? y1 : p.height;
  if (y0 >= y1)                 /* the whole workgroup: an empty trailing zone row, or a short last segment */
    return;
  t_h[threadIdx.x] = 0;
  t_v[threadIdx.x] = 0;
  t_nh[threadIdx.x] = 0;
  t_nv[threadIdx.x] = 0;
  __syncthreads ();

  const int g = (int) (strip * 256u + threadIdx.x);     /* dword of the row */
  if (g < p.row_dwords) {
    const int last = p.row_dwords - 1;
    const int x0 = IN8 ? 4 * g : 2 * g;                 /* its first column: even, < width */
    const bool tail = IN8 && x0 + 2 >= p.width;         /* columns x0 + 2, x0 + 3 are past the row's end */
    const int gl = g > 0 ? g - 1 : g, gr = g < last ? g + 1 : g;        /* 0 .. last: for the address only */
    /* the halves of the lane that have both horizontal neighbours / that exist.  8-bit: the first pair needs columns
     * x0 - 2 and x0 + 2, the second x0 + 4; deep: both columns need dwords g - 1 and g + 1 */
    const uint32_t hmask = IN8 ? (g > 0 && !tail ? 0xffffu : 0u) | (g < last ? 0xffff0000u : 0u)
        : g > 0 && g < last ? 0xffffffffu : 0u;
    const uint32_t vmask = tail ? 0xffffu : 0xffffffffu;
    const uint32_t thr2 = p.thr * 0x10001u;             /* 8-bit: thr <= 510 in both halves */
    uint32_t one = 0x00010001u;
    asm ("" : "+v" (one));      /* dpc_any */
    const uint8_t *sbase = p.src + frame * p.src_frame_bytes;
    /* [row parity][column parity] */
    uint32_t sh[2][2] = {}, sv[2][2] = {}, nh[2][2] = {}, nv[2][2] = {};
    /* row t of the window, y0 - 2 <= t: rows 0 .. height - 1 of this frame only; past the segment's own halo nothing is
     * needed, and the last row asked for is loaded again */
    auto load_row = [&] (int t, uint32_t (&raw)[3]) {
      t = t < y1 + 1 ? t : y1 + 1;
      const int r = t < 0 ? 0 : t >= p.height ? p.height - 1 : t;
      const uint32_t *row = (const uint32_t *) (sbase + (size_t) r * (size_t) p.src_stride);
      raw[0] = row[gl];
      raw[1] = row[g];
      raw[2] = row[gr];
    };
    /* |2 c - a - b| >= thr where `valid`: added to sum[k] and counted in num[k]; a, c, b hold column parity k.  8-bit: in
     * both halves at once; deep: one sample in 32 bits */
    auto add = [&] (uint32_t a, uint32_t c, uint32_t b, uint32_t valid, uint32_t &sum, uint32_t &num) {
      if (IN8) {
        const uint32_t x = c << 1, y = a + b;
        const uint32_t d = dpc_max (x, y) - dpc_min (x, y);
        const uint32_t m = dpc_any (dpc_over (d + 0x00010001u, thr2), one) & valid;
        sum += d & m;
        num += m & 0x00010001u;
      } else {
        const int r = 2 * (int) c - (int) a - (int) b;
        const uint32_t d = (uint32_t) (r < 0 ? -r : r);
        const bool in = valid && d >= p.thr;
        sum += in ? d : 0u;
        num += in ? 1u : 0u;
      }
    };
    /* the row that arrives, of parity rp: its own dword into window row `c`, and -- a row of the segment -- its
     * horizontal responses */
    auto arrive = [&] (const uint32_t (&raw)[3], uint32_t (&c)[NP], int rp, bool own) {
      const uint32_t valid = own ? hmask : 0u;
      if (IN8) {
        const uint32_t l = __builtin_amdgcn_alignbyte (raw[1], raw[0], 2), r = __builtin_amdgcn_alignbyte (raw[2], raw[1], 2);
        c[0] = raw[1] & 0x00ff00ffu;
        c[NP - 1] = (raw[1] >> 8) & 0x00ff00ffu;
        add (l & 0x00ff00ffu, c[0], r & 0x00ff00ffu, valid, sh[rp][0], nh[rp][0]);
        add ((l >> 8) & 0x00ff00ffu, c[NP - 1], (r >> 8) & 0x00ff00ffu, valid, sh[rp][1], nh[rp][1]);
      } else {
        const uint32_t l = __builtin_amdgcn_perm (raw[0], raw[0], p.in_sel) & p.mask2;
        const uint32_t r = __builtin_amdgcn_perm (raw[2], raw[2], p.in_sel) & p.mask2;
        c[0] = __builtin_amdgcn_perm (raw[1], raw[1], p.in_sel) & p.mask2;
        add (l & 0xffffu, c[0] & 0xffffu, r & 0xffffu, valid, sh[rp][0], nh[rp][0]);
        add (l >> 16, c[0] >> 16, r >> 16, valid, sh[rp][1], nh[rp][1]);
      }
    };
    uint32_t w[5][NP], raw[3];
#pragma unroll
    for (int k = 0; k < 5; k++) {
      load_row (y0 - 2 + k, raw);
      arrive (raw, w[k], k & 1, k >= 2 && y0 - 2 + k < y1);
    }
    /* row y, of parity rp, is the middle of the window */
    auto step = [&] (int y, int rp) {
      load_row (y + 3, raw);
      const uint32_t valid = y >= 2 && y + 2 < p.height ? vmask : 0u;
      if (IN8) {
        add (w[0][0], w[2][0], w[4][0], valid, sv[rp][0], nv[rp][0]);
        add (w[0][NP - 1], w[2][NP - 1], w[4][NP - 1], valid, sv[rp][1], nv[rp][1]);
      } else {
        add (w[0][0] & 0xffffu, w[2][0] & 0xffffu, w[4][0] & 0xffffu, valid, sv[rp][0], nv[rp][0]);
        add (w[0][0] >> 16, w[2][0] >> 16, w[4][0] >> 16, valid, sv[rp][1], nv[rp][1]);
      }
#pragma unroll
      for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < NP; j++)
          w[k][j] = w[k + 1][j];
      arrive (raw, w[4], rp ^ 1, y + 3 < y1);
    };
    for (int y = y0; y < y1; y += 2) {  /* uniform over the workgroup; y0 is even: the parities are constants */
      step (y, 0);
      if (y + 1 < y1)
        step (y + 1, 1);
    }
#pragma unroll
    for (int pr = 0; pr < NP; pr++) {   /* the lane's column pairs */
      if (pr == 1 && tail)
        continue;
      const uint32_t zx = fastdiv ((uint32_t) (x0 + 2 * pr), p.div_cw);
#pragma unroll
      for (int site = 0; site < 4; site++) {
        const uint32_t e = zx * 4u + (uint32_t) site;
        const int rp = site >> 1, k = site & 1;
        const uint32_t a = IN8 ? (sh[rp][k] >> (16 * pr)) & 0xffffu : sh[rp][k];
        const uint32_t na = IN8 ? (nh[rp][k] >> (16 * pr)) & 0xffffu : nh[rp][k];
        const uint32_t b = IN8 ? (sv[rp][k] >> (16 * pr)) & 0xffffu : sv[rp][k];
        const uint32_t nb = IN8 ? (nv[rp][k] >> (16 * pr)) & 0xffffu : nv[rp][k];
        if (na) {
          atomicAdd (&t_h[e], (unsigned long long) a);
          atomicAdd (&t_nh[e], na);
        }
        if (nb) {
          atomicAdd (&t_v[e], (unsigned long long) b);
          atomicAdd (&t_nv[e], nb);
        }
      }
    }
  }
  __syncthreads ();
  /* thread t owns table entry t = zone column t / 4, site t % 4 (columns >= zones_x were never added to); a zone is
   * h[4], v[4] (64-bit), nh[4], nv[4] */
  const uint32_t e = threadIdx.x;
  unsigned long long *zone = p.focus
      + 12ull * (((unsigned long long) frame * (uint32_t) p.zones_y + (uint32_t) zy) * (uint32_t) p.zones_x + (e >> 2));
  if (t_nh[e]) {
    atomicAdd (zone + (e & 3u), t_h[e]);
    atomicAdd ((uint32_t *) (zone + 8) + (e & 3u), t_nh[e]);
  }
  if (t_nv[e]) {
    atomicAdd (zone + 4 + (e & 3u), t_v[e]);
    atomicAdd ((uint32_t *) (zone + 10) + (e & 3u), t_nv[e]);
  }
}

hipError_t launch_focus (const FocusParams &p, int nframes, hipStream_t stream)
{
  if (nframes <= 0)
    return nframes == 0 ? hipSuccess : hipErrorInvalidValue;
  if (p.width < 2 || (p.width & 1) || p.height < 1 || p.zones_x < 1 || p.zones_x > kStatsMaxZones || p.zones_y < 1
      || p.ch < 2 || (p.ch & 1) || p.div_cw.d < 2 || (p.div_cw.d & 1)
      || (unsigned long long) p.div_cw.d * (unsigned) p.zones_x < (unsigned) p.width
      || (long long) p.ch * p.zones_y < p.height || (p.in8 && p.thr > 510u))
    return hipErrorInvalidValue;        /* (a zone column past the LDS table, a pair across two zones, a threshold past a half) */
  FocusParams q = p;
  q.row_dwords = p.in8 ? (p.width + 3) / 4 : p.width / 2;
  q.segs = (p.ch + kStatsSegRows - 1) / kStatsSegRows;
  const long long strips = (q.row_dwords + 255) / 256;
  const long long gy = (long long) q.segs * p.zones_y;
  if (strips * nframes > 0x7fffffffLL || gy > 65535)
    return hipErrorInvalidValue;
  q.div_strips = make_fastdiv ((uint32_t) strips);
  const dim3 grid ((unsigned) (strips * nframes), (unsigned) gy);
  if (p.in8)
    hipLaunchKernelGGL (mosaic_focus_kernel<true>, grid, dim3 (256), 0, stream, q);
  else
    hipLaunchKernelGGL (mosaic_focus_kernel<false>, grid, dim3 (256), 0, stream, q);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* stall drill                                                                 */
/* ------------------------------------------------------------------------- */
/* One wave that does nothing for `ticks` ticks of the 100 MHz wall clock: occupies a queue the way a device that
 * has stopped answering does, and ends by itself (mibayer_internal_stall). */
__global__ void __launch_bounds__ (64)
stall_kernel (unsigned long long ticks)
{
  const unsigned long long t0 = wall_clock64 ();
  while (wall_clock64 () - t0 < ticks)
    __builtin_amdgcn_s_sleep (127);
}

hipError_t launch_stall (int ms, hipStream_t stream)
{
  hipLaunchKernelGGL (stall_kernel, dim3 (1), dim3 (64), 0, stream,
      (unsigned long long) ms * 100000ull);
  return hipGetLastError ();
}

/* ------------------------------------------------------------------------- */
/* synthetic mosaic (counter-based, stateless per byte)                        */
/* ------------------------------------------------------------------------- */

__device__ __forceinline__ uint32_t fmix32 (uint32_t z)
{
  z ^= z >> 16;
  z *= 0x85EBCA6Bu;
  z ^= z >> 13;
  z *= 0xC2B2AE35u;
  z ^= z >> 16;
  return z;
}

/* byte(f,y,x) = fmix32((f*H*W + y*W + x) * 2654435761 + seed*0x9E3779B9) & 0xff; padding columns are 0.
 * Grid (x: 16-column groups, y: rows, z: frames): no division anywhere -- the round-1 form decoded a flat index with two
 * 64-bit divisions per dword and took 9.2-10.8 us per 4K frame (0.9 TB/s of stores), as long as the demosaic of that
 * frame (profiles/r06_element_host.md); a thread now writes four dwords of one row, 64 dwords apart. */
__global__ void __launch_bounds__ (256)
fill_synthetic_kernel (uint8_t *buf, int width, int height, int stride,
    unsigned long long frame_bytes, uint32_t first_frame, uint32_t frame0, int y_base, uint32_t seed)
{
  const int y = y_base + (int) (blockIdx.y * blockDim.y + threadIdx.y);
  const uint32_t f = frame0 + blockIdx.z;
  if (y >= height)
    return;
  const uint32_t row_base = (first_frame + f) * (uint32_t) height * (uint32_t) width + (uint32_t) y * (uint32_t) width;
  const uint32_t salt = seed * 0x9E3779B9u;
  uint32_t *row = (uint32_t *) (buf + (unsigned long long) f * frame_bytes + (size_t) y * stride);
  /* four dwords per thread, 64 dwords apart: every wave-store is 256 contiguous bytes */
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const int xd = (int) blockIdx.x * 256 + d * 64 + (int) threadIdx.x;        /* dword in the row */
    const int x = xd * 4;
    if (x >= stride)
      break;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (x + k < width)
        v |= (fmix32 ((row_base + (uint32_t) (x + k)) * 2654435761u + salt) & 0xffu) << (8 * k);
    row[xd] = v;
  }
}

hipError_t launch_fill_synthetic (uint8_t *d_buf, int width, int height,
    int stride, unsigned long long frame_bytes, uint32_t first_frame,
    int nframes, uint32_t seed, hipStream_t stream)
{
  if (nframes <= 0 || height <= 0 || stride <= 0)
    return hipSuccess;
  const dim3 block (64, 4);
  const unsigned gx = (unsigned) (((stride + 15) / 16 + 63) / 64);
  /* rows and frames in chunks the grid's y / z limits (65535) allow */
  for (int y0 = 0; y0 < height; y0 += 65535 * 4) {
    const int rows = height - y0 < 65535 * 4 ? height - y0 : 65535 * 4;
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
      const int nf = nframes - f0 < 65535 ? nframes - f0 : 65535;
      hipLaunchKernelGGL (fill_synthetic_kernel, dim3 (gx, (unsigned) ((rows + 3) / 4), (unsigned) nf), block, 0, stream,
          d_buf, width, height, stride, frame_bytes, first_frame, (uint32_t) f0, y0, seed);
      const hipError_t e = hipGetLastError ();
      if (e != hipSuccess)
        return e;
    }
  }
  return hipSuccess;
}

}  /* namespace mibayer */
