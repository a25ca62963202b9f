/*
 * mibayer.h -- C ABI of the MI355X-native bayer2rgb hot path.
 *
 * This is the drop-in boundary for gst-plugins-bad's `bayer2rgb` element
 * (reference v1.19.2, paths relative to the gst-plugins-bad tree):
 *
 *   the element's per-frame call
 *       gst_bayer2rgb_process (filter, output, frame.info.stride[0],
 *                              map.data, GST_ROUND_UP_4 (filter->width));
 *       gst/bayer/gstbayer2rgb.c:475-477  (body :387-451, row helper :354-381,
 *       ORC inner loops gst/bayer/gstbayerorc.orc:3-248)
 *   is replaced by  mibayer_process_host()  /  mibayer_submit()+mibayer_wait(),
 *   and the per-stream state the reference keeps in struct _GstBayer2RGB
 *   (gstbayer2rgb.c:115-127: width, height, r_off, g_off, b_off, format) is
 *   what mibayer_cfg carries into mibayer_create() from the element's
 *   set_caps vfunc (gstbayer2rgb.c:237-276).
 *
 * Plain C, no GLib / GStreamer / torch types.  All entry points return
 * MIBAYER_OK (0) or a negative mibayer_status; nothing throws across the ABI.
 * There is NO CPU fallback behind this ABI: without a HIP device every
 * compute entry point fails with MIBAYER_ERR_NO_DEVICE.
 *
 * Output is bit-exact (uint8) with the reference CPU/ORC path for every
 * geometry in which the reference is well defined: even width >= 4 and
 * height >= 3 (odd widths leave the last column unwritten and read
 * uninitialised scratch in the reference; height < 3 reads uninitialised or
 * out-of-bounds rows -- gstbayer2rgb.c:365-380, :430-447).  Anything else is
 * rejected with MIBAYER_ERR_GEOMETRY at mibayer_create() time.
 */
#ifndef MIBAYER_H
#define MIBAYER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: additive over 1 -- pool failover / fault injection / helper threads,
 * mibayer_process_device_list, mibayer_host_alloc_near + NUMA queries,
 * mibayer_dev_stream_* / mibayer_dev_upload_async / mibayer_dev_event_query;
 * MIBAYER_FLAG_HIPGRAPH now captures the compute-queue segment of a frame.
 * Every v1 entry point keeps its signature and meaning. */
/* 3: additive over 2 -- deadlines on every host-side wait (MIBAYER_ERR_TIMEOUT,
 * mibayer_set_wait_timeout, mibayer_pool_set_wait_timeout); mibayer_sync /
 * mibayer_destroy wait for the context's own frames only. */
/* 4: additive over 3 -- the launch plan as a value (mibayer_get_plan / mibayer_set_plan /
 * mibayer_plan_source), the process-wide plan cache behind mibayer_autotune and
 * mibayer_create (mibayer_plan_cache_clear), mibayer_autotune_list, the host-wait
 * policy (mibayer_set_wait_spin), MIBAYER_FLAG_HIPGRAPH_CHAIN, mibayer_is_lab_build. */
/* NOTE on 4: the numeric kernel-variant ids were renumbered in that version (4 used to be lds_1x8_r4_dpp and became
 * lds_4x2_r4_dpp; the former 20-24 became 4-9; ids >= 10 exist in the lab build only) -- the one non-additive change
 * of the ABI's history.  Every id is bit-exact, so a caller that kept a number got a different speed, not different
 * bytes, or MIBAYER_ERR_ARG for an id the product build no longer has.  Look variants up by NAME
 * (mibayer_variant_name) rather than keeping numbers across versions. */
/* 5: additive over 4 -- one launch plan per LAUNCH CLASS (launches of a few rounds of workgroups: one frame per
 * launch, vs. batch launches): mibayer_get_plan_for / mibayer_set_plan_for, the plan cache keyed by class;
 * mibayer_ctx_frame_queue (four compute queues per device on hardware queues of their own, for independent one-frame
 * launches), covered by mibayer_sync;
 * mibayer_device_pci_bus_id.
 * mibayer_get_plan / mibayer_plan_source / mibayer_ctx_variant_name keep describing the batch-class plan,
 * mibayer_set_plan / mibayer_copy_plan pin every class. */
/* 5, later additive: deep samples -- flags only (MIBAYER_FLAG_SRC_BITS, _SRC_BIG_ENDIAN, _DST_16BIT,
 * _DST_BIG_ENDIAN: 10-16-bit mosaics in 16-bit words, 16-bit-per-channel output); no struct field and no entry point
 * was added, and a cfg without them means what it meant.  Likewise MIBAYER_FLAG_MHC (Malvar-He-Cutler demosaic). */
/* 5, later additive: the fused colour stage -- MIBAYER_FLAG_COLOUR, struct mibayer_colour and the entry points of
 * group `colour`; a cfg without the flag means what it meant. */
/* 5, later additive: mosaic zone statistics -- struct mibayer_stats_zone and the entry points of group `stats`. */
/* 5, later additive: mosaic histogram -- struct mibayer_hist and the entry points of group `hist`. */
/* 5, later additive: packed 24-bit output -- MIBAYER_FLAG_DST_24BIT, a fifth deep flag; no struct field and no entry
 * point was added, and a cfg without the flag means what it meant. */
/* 5, later additive: planar 8-bit output -- MIBAYER_FLAG_DST_PLANAR, a sixth deep flag; no struct field and no entry
 * point was added, and a cfg without the flag means what it meant. */
/* 5, later additive: lens shading correction -- struct mibayer_shading and the entry points of group `shading`; a
 * context without a table converts what it converted. */
/* 5, later additive: defective pixel correction -- struct mibayer_dpc and the entry points of group `dpc`; a context
 * with the correction off converts what it converted. */
/* 5, later additive: noise reduction -- struct mibayer_nr and the entry points of group `nr`; a context with the curve
 * off converts what it converted. */
/* 5, later additive: mosaic focus statistics -- struct mibayer_focus_zone and the entry points of group `focus`. */
/* 5, later additive: half-size demosaic -- MIBAYER_FLAG_HALF, a flag only; no struct field and no entry point was
 * added, and a cfg without the flag means what it meant. */
#define MIBAYER_ABI_VERSION 5

/* MIBAYER ABI GROUPS -- which of the entry points are the drop-in and which are not.  The ABI is
 * FROZEN at version 5: round 6 added nothing.  A maintainer who replaces gst_bayer2rgb_process needs `core` only
 * (INTEGRATION.md section 2 uses create / process_host / destroy / strerror); everything else serves a named
 * consumer and can be ignored by anybody who is not that consumer.  The dynamic symbol table of libmibayer.so is
 * exactly this list (linker version script generated from this header; tests/test_abi.py checks both).
 *
 * group core: the boundary SURVEY.md section 8(b) proposed -- context, one frame host->host (synchronous and queued),
 *   a device-resident batch, pinned host memory
 *     mibayer_abi_version mibayer_device_count mibayer_strerror mibayer_last_hip_error mibayer_create mibayer_destroy
 *     mibayer_get_cfg mibayer_process_host mibayer_submit mibayer_wait mibayer_pending mibayer_process_device
 *     mibayer_sync mibayer_host_alloc mibayer_host_free
 * group sharding: frames round-robin over the GPUs of a node, with failover (north_star; bayer2rgb devices=...)
 *     mibayer_pool_create mibayer_pool_destroy mibayer_pool_capacity mibayer_pool_pending mibayer_pool_submit
 *     mibayer_pool_wait mibayer_pool_alive mibayer_pool_take_failure mibayer_pool_reclaim mibayer_pool_lost
 * group device-memory: what plugin `mihip` (memory:HIPMemory elements) and bench.py are built on --
 *   device allocations, copies, streams and events without a context, list launches, the synthetic-frame generator
 *     mibayer_process_device_list mibayer_ctx_stream mibayer_ctx_frame_queue mibayer_device_alloc mibayer_device_free
 *     mibayer_copy_to_device mibayer_copy_from_device mibayer_dev_alloc mibayer_dev_free mibayer_dev_upload
 *     mibayer_dev_download mibayer_dev_stream_create mibayer_dev_stream_destroy mibayer_dev_upload_async
 *     mibayer_dev_download_async mibayer_dev_event_query mibayer_dev_event_create mibayer_dev_event_destroy
 *     mibayer_dev_event_record mibayer_dev_event_wait mibayer_dev_stream_wait_event mibayer_host_alloc_near
 *     mibayer_host_is_pinned mibayer_device_numa_node mibayer_host_numa_node mibayer_fill_synthetic
 * group tuning: launch plans (measured / cached / set), wait policy and deadlines -- every one of them has a default
 *     mibayer_autotune mibayer_autotune_list mibayer_copy_plan mibayer_get_plan mibayer_set_plan mibayer_get_plan_for
 *     mibayer_set_plan_for mibayer_plan_source mibayer_plan_from_cache mibayer_plan_cache_clear mibayer_time_device
 *     mibayer_set_wait_timeout mibayer_set_wait_spin mibayer_pool_set_wait_timeout mibayer_pool_set_wait_spin
 * group diagnostics: what tests, bench.py and the drills read -- never needed to convert a frame
 *     mibayer_is_lab_build mibayer_device_pci_bus_id mibayer_get_host_stats mibayer_pool_get_host_stats
 *     mibayer_pool_inject_fault mibayer_pool_inject_stall mibayer_deferred_frees mibayer_wedged_contexts
 *     mibayer_variant_count mibayer_variant_name mibayer_auto_variant mibayer_frame_class_variant
 *     mibayer_known_width_plan mibayer_ctx_variant_name mibayer_plan_selectors mibayer_launch_geometry
 *     mibayer_block_to_tile
 * group focus: the third measurement of the ISP statistics block -- per-zone sums and counts of the same-site second
 *   differences of the mosaic (sharpness), and the score that auto focus reads
 *     mibayer_focus_device mibayer_set_focus mibayer_frame_focus mibayer_pool_set_focus mibayer_pool_frame_focus
 *     mibayer_focus_score
 * group nr: noise reduction -- a sigma filter over the 24 same-site neighbours of every sample of the mosaic, its
 *   threshold a curve over the sample's level, behind the defect pass and before everything else reads the mosaic
 *     mibayer_set_nr mibayer_get_nr mibayer_nr_device mibayer_pool_set_nr mibayer_nr_curve
 * group dpc: defective pixel correction -- stuck samples of the mosaic, found by threshold against their same-site
 *   neighbours or named in a list, replaced from the flattest neighbour pair before everything else reads them
 *     mibayer_set_dpc mibayer_get_dpc mibayer_dpc_device mibayer_pool_set_dpc
 * group shading: lens shading correction -- a per-site gain grid applied to the mosaic before everything else reads it,
 *   and the helper that turns flat-field zone statistics into such a grid
 *     mibayer_shading_nodes mibayer_set_shading mibayer_get_shading mibayer_shade_device mibayer_pool_set_shading
 *     mibayer_stats_shading
 * group hist: the other half of the ISP statistics block -- a 256-bin histogram per CFA site of the mosaic, and the
 *   percentile and auto-exposure helpers that read it
 *     mibayer_hist_device mibayer_set_hist mibayer_frame_hist mibayer_pool_set_hist mibayer_pool_frame_hist
 *     mibayer_hist_percentile mibayer_hist_exposure
 * group stats: the ISP statistics block -- per-zone sums and counts per CFA site of the mosaic, and grey-world white balance
 *     mibayer_stats_device mibayer_set_stats mibayer_frame_stats mibayer_pool_set_stats mibayer_pool_frame_stats
 *     mibayer_stats_grey_world
 * group colour: the opt-in colour stage fused into the demosaic (MIBAYER_FLAG_COLOUR): black level, matrix, tone curve
 *     mibayer_colour_init mibayer_set_colour mibayer_get_colour mibayer_pool_set_colour mibayer_colour_matrix
 *     mibayer_colour_tone
 * END OF MIBAYER ABI GROUPS */

/* Bayer order; numbering identical to the reference's anonymous enum
 * GST_BAYER_2_RGB_FORMAT_*, gstbayer2rgb.c:95-101. */
typedef enum mibayer_pattern {
  MIBAYER_BGGR = 0,
  MIBAYER_GBRG = 1,
  MIBAYER_GRBG = 2,
  MIBAYER_RGGB = 3
} mibayer_pattern;

typedef enum mibayer_status {
  MIBAYER_OK = 0,
  MIBAYER_ERR_ARG = -1,         /* NULL pointer, bad struct_size, bad enum   */
  MIBAYER_ERR_GEOMETRY = -2,    /* width/height/stride outside the domain    */
  MIBAYER_ERR_LAYOUT = -3,      /* (r,g,b)_off is none of the 4 byte layouts
                                   the reference has merge functions for
                                   (gstbayer2rgb.c:409-421)                  */
  MIBAYER_ERR_NO_DEVICE = -4,   /* no HIP device / ordinal out of range      */
  MIBAYER_ERR_HIP = -5,         /* a HIP runtime call failed                 */
  MIBAYER_ERR_NOMEM = -6,
  MIBAYER_ERR_BUSY = -7,        /* async ring full: call mibayer_wait()      */
  MIBAYER_ERR_EMPTY = -8,       /* mibayer_wait() with nothing in flight     */
  MIBAYER_ERR_TIMEOUT = -9      /* the device did not complete a frame within
                                   the wait deadline (mibayer_set_wait_timeout);
                                   the context is wedged: every later call
                                   returns this at once -- until the device has
                                   caught up with what the context had queued
                                   (polled, never waited for), then the context
                                   works again and its frames can be collected */
} mibayer_status;

/* Per-stream configuration == the fields of struct _GstBayer2RGB
 * (gstbayer2rgb.c:115-127) plus the strides gst_bayer2rgb_transform passes
 * (:475-477) and where to run. */
typedef struct mibayer_cfg {
  uint32_t struct_size;   /* = sizeof (mibayer_cfg)                          */
  int32_t width;          /* pixels; even, >= 4                              */
  int32_t height;         /* rows; >= 3                                      */
  int32_t src_stride;     /* bytes per mosaic row; 0 = GST_ROUND_UP_4(width),
                             the value the reference always passes (:477);
                             must be a multiple of 4 and >= ROUND_UP_4(width) */
  int32_t dst_stride;     /* bytes per output row; 0 = 4*width; multiple of 4,
                             >= 4*width (GstVideoMeta may pad, :476)         */
  int32_t pattern;        /* mibayer_pattern                                 */
  int32_t r_off;          /* byte index of R, G, B inside the 4-byte output  */
  int32_t g_off;          /* pixel == GST_VIDEO_INFO_COMP_OFFSET (info, 0..2) */
  int32_t b_off;          /* (:268-271).  The 4th byte is written as 255.    */
  int32_t device;         /* HIP device ordinal; -1 = the current device     */
  int32_t inflight;       /* host path: frames in flight (ring depth) for
                             mibayer_submit(); 0 = default (2)               */
  int32_t variant;        /* kernel variant; 0 = default.  Tuning knob, every
                             variant is bit-exact            */
  uint32_t flags;         /* MIBAYER_FLAG_* or 0.  Deep samples (16-bit-word
                             mosaics, 16-bit channels) are flags too, and
                             change the stride defaults / units above and the
                             offsets to 16-bit channels: MIBAYER_FLAG_SRC_BITS */
} mibayer_cfg;

/* Host path: the compute-queue segment of every frame (wait for the upload ->
 * kernel -> signal the download) is captured once per ring slot as a hipGraph
 * and replayed with one hipGraphLaunch per frame; the pinned H2D / D2H copies
 * stay asynchronous copies on the two copy queues (BASELINE.json configs[4]:
 * "pinned double-buffered H2D/D2H + hipGraph-captured launch"). */
#define MIBAYER_FLAG_HIPGRAPH 1u

/* Inverse direction, the plugin's sibling element rgb2bayer (reference
 * gst/bayer/gstrgb2bayer.c:230-278): the source is 4 B/pixel (src_stride
 * default 4*width), the destination the 8-bit mosaic (dst_stride default
 * ROUND_UP_4(width), :179/:255); output byte (j,i) = the R, G or B byte of input
 * pixel (j,i) selected by the CFA site, with (r_off,g_off,b_off) = byte offsets
 * inside the INPUT pixel (the reference accepts ARGB only: 1,2,3).  Any
 * width/height >= 1.  Every host/device/pool entry point works unchanged;
 * variant must be 0; mibayer_autotune / mibayer_fill_synthetic do not apply. */
#define MIBAYER_FLAG_RGB2BAYER 2u

/* With MIBAYER_FLAG_HIPGRAPH: the WHOLE upload -> kernel -> download chain of a
 * ring slot as one graph on the slot's own queue (the host pointers are patched
 * into the instantiated graph per frame) instead of the compute-queue segment
 * only.  Measured slower at 4K (the copies of consecutive frames serialise per
 * slot); kept as the A/B arm bench.py reports. */
#define MIBAYER_FLAG_HIPGRAPH_CHAIN 4u

/* Deep samples (additive within version 5: flags only, mibayer_cfg keeps its fields).  A context with any of the
 * four flags below, or MIBAYER_FLAG_DST_24BIT or MIBAYER_FLAG_DST_PLANAR (paragraphs of their own further down), is a
 * DEEP context; the algorithm
 * is the one of the 8-bit path on wider integers:
 *   input   one 16-bit word per sample (little-endian; big-endian with MIBAYER_FLAG_SRC_BIG_ENDIAN), masked to its
 *           low `bits` bits -- everything above them is ignored; MIBAYER_FLAG_SRC_BITS(0) = the 8-bit mosaic;
 *   average avg(a,b) = (a+b+1)>>1 on the masked values, at the native depth; nothing is rescaled before the end;
 *   output  16-bit channels (MIBAYER_FLAG_DST_16BIT, 8-byte pixels): v << (16 - bits), alpha 0xffff, little-endian
 *           words (big-endian with MIBAYER_FLAG_DST_BIG_ENDIAN); r_off / g_off / b_off count 16-bit CHANNELS 0..3
 *           in the four layouts of the 8-bit path (ARGB64 = 1,2,3).  Without DST_16BIT the 4-byte formats:
 *           v >> (bits - 8), truncating, alpha 255.  An 8-bit mosaic with 16-bit output is v << 8.
 * Strides: 16-bit samples src_stride default 2*width, >= 2*width, multiple of 4; DST_16BIT dst_stride default
 * 8*width, >= 8*width, multiple of 8.  Device-path base pointers (d_src, d_dst, every entry of a list) and the frame
 * pitches of a batch need only be multiples of 4, whatever the strides, in a deep, MHC or COLOUR context alike -- the
 * kernels' vector loads and stores ask for dword alignment only -- so a source at 4 mod 8 and an 8-byte-pixel
 * destination at 4 mod 8 are valid; anything else is MIBAYER_ERR_ARG (MIBAYER_ERR_GEOMETRY for a pitch).
 * Geometry as the 8-bit path (even width >= 4, height >= 3).  Any of the four
 * together with MIBAYER_FLAG_RGB2BAYER, SRC_BITS outside {0, 10, 12, 14, 16} or an endianness flag without its
 * depth is MIBAYER_ERR_ARG.  Every host / device / list / pool entry point works on a deep context; the host path
 * accepts MIBAYER_FLAG_HIPGRAPH and runs without graphs (as rgb2bayer does).  mibayer_autotune[_list],
 * mibayer_fill_synthetic, mibayer_set_plan[_for] and mibayer_plan_selectors return MIBAYER_ERR_ARG: a deep context
 * has one kernel shape and no plans. */
#define MIBAYER_FLAG_SRC_BITS(n) ((uint32_t) (n) << 8)
#define MIBAYER_FLAG_SRC_BITS_MASK (0x1fu << 8)
#define MIBAYER_FLAG_SRC_BIG_ENDIAN (1u << 13)
#define MIBAYER_FLAG_DST_16BIT (1u << 14)
#define MIBAYER_FLAG_DST_BIG_ENDIAN (1u << 15)

/* Packed 24-bit output (additive within version 5: a flag only): 3-byte pixels, RGB or BGR, what tensor preprocessing,
 * encoders and image writers take -- no pad byte written, and no second pass to drop it.  A fifth deep flag: a context
 * that carries it is a DEEP context and everything said of deep contexts above holds (one kernel shape, no plans, variant
 * must be 0; MIBAYER_FLAG_HIPGRAPH is accepted and the host path runs without graphs; mibayer_autotune[_list],
 * mibayer_set_plan[_for], mibayer_plan_selectors and mibayer_launch_geometry return MIBAYER_ERR_ARG), except that
 * mibayer_fill_synthetic works when the mosaic is 8-bit; mibayer_ctx_variant_name names the strip kernel.
 *   output  the R, G and B bytes of the SAME cfg with RGBx (0,1,2) or BGRx (2,1,0) and without the flag, byte 3 dropped:
 *           the reference's bytes for an 8-bit mosaic, v >> (bits - 8) for deep mosaics, the MHC filters' and the colour
 *           stage's o >> 8 alike.  (r_off, g_off, b_off) = (0,1,2) is RGB, (2,1,0) is BGR; anything else is
 *           MIBAYER_ERR_LAYOUT.
 *   strides dst_stride default ROUND_UP_4 (3*width), GStreamer's RGB stride; >= 3*width and a multiple of 4.  Only the
 *           first 3*width bytes of a row are written, on the device paths and on the host path alike: with
 *           width % 4 == 2 the row ends two bytes before the default stride, and those two bytes (like every byte of a
 *           wider stride's padding) keep what they held.  Device pointers and frame pitches: multiples of 4, as above.
 * Goes with MIBAYER_FLAG_SRC_BITS (10/12/14/16), _SRC_BIG_ENDIAN, MIBAYER_FLAG_MHC, MIBAYER_FLAG_COLOUR and the
 * statistics; with MIBAYER_FLAG_DST_16BIT, _DST_BIG_ENDIAN or MIBAYER_FLAG_RGB2BAYER it is MIBAYER_ERR_ARG.  Geometry
 * as the 8-bit path (even width >= 4, height >= 3), width <= 2^26 as for the other deep flags.  A plain 8-bit bilinear
 * context with the flag runs the strip kernel instead of the production kernels; its bytes are theirs.  (Bit 21: bits
 * 17, 18 and 20 stay unknown flags, MIBAYER_ERR_ARG, as they have been.) */
#define MIBAYER_FLAG_DST_24BIT (1u << 21)

/* Planar 8-bit output (additive within version 5: a flag only): three planes of 8-bit samples, (3, height, width) as
 * tensor code takes it (NCHW) -- no interleaved frame written, and no second pass to transpose it.  A sixth deep flag:
 * a context that carries it is a DEEP context and everything said of deep contexts above holds (one kernel shape, no
 * plans, variant must be 0; MIBAYER_FLAG_HIPGRAPH is accepted and the host path runs without graphs; mibayer_autotune[_list],
 * mibayer_set_plan[_for], mibayer_plan_selectors and mibayer_launch_geometry return MIBAYER_ERR_ARG), except that
 * mibayer_fill_synthetic works when the mosaic is 8-bit; mibayer_ctx_variant_name names the strip kernel.
 *   output  a frame is three planes, each `height` rows of dst_stride bytes; plane k starts at
 *           dst + k * dst_stride * height (the plane pitch is not configurable: GStreamer's GBR / RGBP / BGRP layout).
 *           (r_off, g_off, b_off) are the PLANE INDICES of R, G and B, any permutation of (0, 1, 2): RGBP = (0,1,2),
 *           BGRP = (2,1,0), GBR = (2,0,1); anything else is MIBAYER_ERR_LAYOUT.
 *   values  byte (y, x) of the R plane is byte 0 of pixel (y, x) of the SAME cfg with RGBx (0,1,2) and without the
 *           flag, G is byte 1, B is byte 2: the reference's bytes for bilinear on an 8-bit mosaic, v >> (bits - 8) for deep
 *           mosaics, the MHC filters' and the colour stage's o >> 8 alike.
 *   strides dst_stride default ROUND_UP_4 (width); >= width and a multiple of 4, else MIBAYER_ERR_GEOMETRY.  Only the
 *           first `width` bytes of a row of a plane are written, on the device paths and on the host path alike: with
 *           width % 4 == 2 a row ends two bytes before the default stride, and those two bytes (like every byte of a
 *           wider stride's padding) keep what they held.
 *   sizes   a frame is 3 * dst_stride * height bytes: what a batch's dst_frame_bytes must at least be, what the host
 *           path's `dst` holds, and where d_dsts[f] of a list launch points (the base of frame f's three planes).
 *           Device pointers and frame pitches: multiples of 4, as above.
 * Goes with MIBAYER_FLAG_SRC_BITS (10/12/14/16), _SRC_BIG_ENDIAN, MIBAYER_FLAG_MHC, MIBAYER_FLAG_COLOUR and the
 * statistics; with MIBAYER_FLAG_DST_16BIT, _DST_BIG_ENDIAN, MIBAYER_FLAG_DST_24BIT or MIBAYER_FLAG_RGB2BAYER it is
 * MIBAYER_ERR_ARG (16-bit planes do not exist yet).  Geometry as the 8-bit path (even width >= 4, height >= 3),
 * width <= 2^26 as for the other deep flags.  A plain 8-bit bilinear context with the flag runs the strip kernel
 * instead of the production kernels; its bytes are theirs.  (Bit 22: bits 17, 18, 20, 24 and 31 stay unknown flags.) */
#define MIBAYER_FLAG_DST_PLANAR (1u << 22)

/* Malvar-He-Cutler demosaic (additive within version 5: a flag only).  Instead of the reference's bilinear average, the
 * gradient-corrected linear interpolation of Malvar, He and Cutler (ICASSP 2004): fewer zipper artefacts and colour
 * fringes on edges, NOT bit-exact with gst-plugins-bad.  S = the sample as the deep path reads it (8-bit byte, or the
 * word in its byte order masked to `bits`), depth = 8 or `bits`.  Borders reflect-101 (index -1 -> 1, -2 -> 2,
 * W -> W-2, W+1 -> W-3, rows alike).  The filters, x16 so that they are integers, by offset (dy,dx):
 *   F_G    green at an R / B site:          (0,0) 8; (0,+-1),(+-1,0) 4; (0,+-2),(+-2,0) -2
 *   F_row  the colour left/right of a G:    (0,0) 10; (0,+-1) 8; (0,+-2) -2; (+-1,+-1) -2; (+-2,0) +1
 *   F_col  the colour above/below a G:      F_row transposed
 *   F_diag R at a B site / B at an R site:  (0,0) 12; (+-1,+-1) 4; (0,+-2),(+-2,0) -3
 * R site: R = S, G = F_G, B = F_diag; B site: B = S, G = F_G, R = F_diag; G site: G = S and F_row / F_col for the
 * colours of its row / column.  v = clamp ((acc + 8) >> 4, 0, 2^depth - 1) on int32 sums, then the deep path's output
 * conversion and layouts.  Goes with any of the deep flags above and with MIBAYER_FLAG_HIPGRAPH (the host path runs
 * without graphs); with MIBAYER_FLAG_RGB2BAYER or variant != 0 it is MIBAYER_ERR_ARG.  Strides and their defaults are
 * those of the same cfg without the flag.  Every host / device / list / pool entry point works on an MHC context;
 * mibayer_autotune[_list], mibayer_set_plan[_for], mibayer_plan_selectors and mibayer_launch_geometry return
 * MIBAYER_ERR_ARG (one kernel shape, no plans); mibayer_fill_synthetic works when the mosaic is 8-bit;
 * mibayer_ctx_variant_name names the MHC kernel. */
#define MIBAYER_FLAG_MHC (1u << 16)

/* Fused colour stage (additive within version 5: a flag, a struct and the entry points of group `colour`).  What the
 * demosaic leaves is sensor-space data; a COLOUR context subtracts the black level, applies a 3x3 matrix (white
 * balance x colour correction) and optionally a tone curve inside the demosaic kernel, on the values it holds in
 * registers -- no second pass over the frame.  depth = 8 or `bits`, max = 2^depth - 1, (R, G, B) = the demosaiced values
 * at native depth, exactly what the deep or MHC path computes before its output conversion.  Per pixel, in integers:
 *   1. c = max (c - black[k], 0)                                           k = R, G, B; black[k] in 0 .. 65535
 *   2. acc_k = m[3k] R + m[3k+1] G + m[3k+2] B  (exact)                    Q12: 4096 = 1.0, entries in -65535 .. 65535
 *      c'_k = clamp ((acc_k + 2048) >> 12, 0, max)                         arithmetic shift
 *   3. with a tone curve (has_tone, tone[257], entries in 0 .. 65536):
 *        t = c' << (16 - depth), i = t >> 8, f = t & 255
 *        o = min ((tone[i] (256 - f) + tone[i+1] f + 128) >> 8, 65535)
 *      16-bit channels take o, 8-bit channels o >> 8; without a curve the deep path's output conversion applies to c'
 *   4. alpha, byte orders and the four layouts as without the flag.
 * Zero black level, the identity matrix and no curve give the bytes of the same cfg without the flag; tone[i] = 256 i on
 * top leaves 16-bit output unchanged.  The flag goes with every deep flag, with MIBAYER_FLAG_MHC and with
 * MIBAYER_FLAG_HIPGRAPH (the host path runs without graphs); with MIBAYER_FLAG_RGB2BAYER or variant != 0 it is
 * MIBAYER_ERR_ARG.  Geometry, strides and layouts are those of the same cfg without the flag.  Like a deep or MHC
 * context a colour context has one kernel shape and no plans: mibayer_autotune[_list], mibayer_set_plan[_for],
 * mibayer_plan_selectors and mibayer_launch_geometry return MIBAYER_ERR_ARG; mibayer_fill_synthetic works when the
 * mosaic is 8-bit; mibayer_ctx_variant_name names the colour kernel. */
#define MIBAYER_FLAG_COLOUR (1u << 19)

typedef struct mibayer_colour {
  uint32_t struct_size;         /* = sizeof (mibayer_colour) */
  int32_t black[3];             /* R, G, B, at native depth */
  int32_t matrix[9];            /* row-major, Q12: output channel k = row k */
  int32_t has_tone;             /* 0 / 1 */
  uint32_t tone[257];
} mibayer_colour;

#define MIBAYER_TONE_LINEAR 0   /* tone[i] = 256 i */
#define MIBAYER_TONE_SRGB 1     /* the sRGB transfer function (IEC 61966-2-1) */
#define MIBAYER_TONE_GAMMA 2    /* x ^ (1 / gamma), gamma in 0.01 .. 100 */

typedef struct mibayer_ctx mibayer_ctx;
typedef struct mibayer_pool mibayer_pool;

/* the identity: zero black level, matrix 4096 on the diagonal, no tone curve */
void mibayer_colour_init (mibayer_colour *colour);
/* Sets / reads the stage of a COLOUR context (a new one holds the identity).  MIBAYER_ERR_ARG on a context without
 * the flag and on out-of-range values.  May be called between frames, from any thread: it applies to the frames
 * accepted (mibayer_submit / mibayer_process_host) and the device-path calls made after it returns, never to ones
 * already queued.  A host-path frame takes ONE copy of the parameters when it is accepted, whatever number of bands
 * it is launched in, a mibayer_process_device[_list] call one per call; the copy, tone table included, travels in the
 * kernel arguments. */
int mibayer_set_colour (mibayer_ctx *ctx, const mibayer_colour *colour);
int mibayer_get_colour (const mibayer_ctx *ctx, mibayer_colour *out);
/* ... of a pool: the stage of the frames mibayer_pool_submit accepts after it returns.  The pool keeps the stage with
 * each frame and gives it to a shard's context only together with the frame, so frames that still wait in a shard's
 * helper thread keep the parameters they were submitted with, and so does a frame that is converted again on a
 * surviving device after a failover.  Call it from the thread that calls mibayer_pool_submit.  MIBAYER_ERR_ARG on a
 * pool without the flag and on out-of-range values. */
int mibayer_pool_set_colour (mibayer_pool *pool, const mibayer_colour *colour);
/* Pure host helpers (no device needed), so that every caller rounds alike.  out = round (ccm x diag (gains) x 4096):
 * white-balance gains per input channel (R, G, B) under a colour-correction matrix (NULL = identity);
 * MIBAYER_ERR_ARG when an entry leaves -65535 .. 65535. */
int mibayer_colour_matrix (const double gains[3], const double ccm[9], int32_t out[9]);
/* tone[i] = round (65536 f (i / 256)) for MIBAYER_TONE_*; `gamma` is read by MIBAYER_TONE_GAMMA only */
int mibayer_colour_tone (int curve, double gamma, uint32_t tone[257]);

/* ---- half-size demosaic (additive within version 5: a flag only) -------------------------------------------------- */

/* One RGB pixel per CFA quad (dcraw -h, LibRaw half_size): a quarter of the pixels, each built from the four samples of
 * its own quad only -- nothing interpolated, no neighbourhood, no border rule.  What previews, analytics and tensor
 * ingest take, without a full demosaic and a scaler behind it.
 *   geometry  cfg.width / cfg.height stay the MOSAIC's (W, H) under the usual rules: even W >= 4, H >= 3, W <= 2^26.
 *             The output is OW = W / 2 by OH = H >> 1 pixels; the last row of an odd height has no quad and is dropped.
 *             OW may be odd (W = 6 -> 3).
 *   samples   S, masking, byte order and depth exactly as in group `stats`.  Output pixel (X, Y) reads S (2X + dx,
 *             2Y + dy), dx, dy in {0, 1}: R = the quad's red sample, B = its blue one, G = (Ga + Gb + 1) >> 1 of its
 *             two green samples at native depth; the Bayer order says which is which.  The pixel sits at the quad's
 *             CENTRE: R and B are each half an output pixel (one sample) off it, in opposite directions.
 *   output    from (R, G, B) on everything is the deep path's: v >> (bits - 8) for 8-bit channels, v << (16 - bits) for
 *             16-bit ones, alpha, the four 4-byte layouts, MIBAYER_FLAG_DST_16BIT / _DST_BIG_ENDIAN, _DST_24BIT and
 *             _DST_PLANAR; with MIBAYER_FLAG_COLOUR steps 1-4 of the stage run verbatim on (R, G, B).
 *   strides   dst_stride default ROUND_UP_4 (px * OW), px = the bytes of a pixel in a row (4 / 8 / 3 / 1); >= px * OW and
 *             a multiple of 4 (8 for 16-bit channels), else MIBAYER_ERR_GEOMETRY.  Only the first px * OW bytes of a
 *             row are written.  src_stride as without the flag.
 *   sizes     a frame is dst_stride * OH bytes, x 3 when planar (plane k at dst + k * dst_stride * OH): what a batch's
 *             dst_frame_bytes must at least be, where d_dsts[f] points and what the host path's `dst` holds.
 * With MIBAYER_FLAG_MHC (there is nothing to interpolate), MIBAYER_FLAG_RGB2BAYER or variant != 0 it is MIBAYER_ERR_ARG;
 * MIBAYER_FLAG_HIPGRAPH is accepted and the host path runs without graphs.  A HALF context has one kernel shape and no
 * plans, like a deep context: mibayer_autotune[_list], mibayer_set_plan[_for], mibayer_plan_selectors and
 * mibayer_launch_geometry return MIBAYER_ERR_ARG; mibayer_fill_synthetic works when the mosaic is 8-bit;
 * mibayer_ctx_variant_name names the half-size kernel.  The host path launches each frame whole (no bands).  Groups
 * `stats`, `hist`, `focus`, `shading`, `dpc` and `nr` work on the mosaic and are unchanged: grids, windows and limits in
 * source coordinates, and on the host path they run before the half-size launch as before the full one.
 * (Bit 23: bits 17, 18, 20, 24 and 31 stay unknown flags.) */
#define MIBAYER_FLAG_HALF (1u << 23)

/* ---- mosaic zone statistics (additive within version 5: a struct and the entry points of group `stats`) -------- */

/* What an ISP's statistics block hands to auto white balance and exposure: sums and counts per CFA site over a grid of
 * zones, measured on the MOSAIC (before the demosaic and the colour stage) by a read-only kernel.
 *   sample   S = what the deep path reads: the byte of an 8-bit mosaic, or the 16-bit word in the context's byte order
 *            masked to `bits`; depth = 8 or `bits`, max = 2^depth - 1
 *   site     s = 2 (y & 1) + (x & 1); its colour by Bayer order: bggr B G G R, gbrg G B R G, grbg G R B G, rggb R G G B
 *   zones    a grid of zones_x x zones_y, each 1 .. 64, zones_x <= W/2 and zones_y <= H/2; a cell is
 *            cw = 2 ceil ((W/2) / zones_x) pixels wide and ch = 2 ceil ((H/2) / zones_y) rows high (H/2 exact, not
 *            rounded down: the last row of an odd height has a zone), pixel (x, y) belongs to zone (x / cw, y / ch);
 *            trailing zones may be empty and are then all zero
 * Only columns < W count: stride padding and the bits above `bits` are ignored.  Everything is an integer, so the result
 * does not depend on the order of the kernel's atomic additions. */
typedef struct mibayer_stats_zone {     /* 64 bytes */
  uint64_t sum[4];              /* sum of S over the samples of site s with lo <= S <= hi */
  uint32_t count[4];            /* their number */
  uint32_t clipped[4];          /* samples of site s with S > hi */
} mibayer_stats_zone;
#define MIBAYER_STATS_MAX_ZONES 64      /* per direction */

/* Device path: zeroes d_stats (nframes * zones_y * zones_x zones, frame-major, then row-major) on `hip_stream`, then
 * ONE launch over the batch, frame f read at d_src + f * src_frame_bytes as by mibayer_process_device.  Valid on every
 * bayer2rgb context (8-bit, deep, MHC, COLOUR).  MIBAYER_ERR_ARG on an RGB2BAYER context, lo > hi, hi > max, a grid
 * outside the rule above, d_src not a multiple of 4 or d_stats not a multiple of 8; MIBAYER_ERR_GEOMETRY for a frame
 * pitch as in mibayer_process_device.  Covered by mibayer_sync when launched on the context's stream. */
int mibayer_stats_device (mibayer_ctx *ctx, const void *d_src, size_t src_frame_bytes, int nframes, int zones_x,
    int zones_y, uint32_t lo, uint32_t hi, mibayer_stats_zone *d_stats, void *hip_stream);
/* Host path: every frame accepted (mibayer_submit / mibayer_process_host) after this returns also gets its statistics,
 * computed on the device copy of the mosaic that its ring slot holds anyway -- every row once, however many bands the
 * frame is launched in -- and downloaded with the frame into pinned memory of the slot.  (0, 0) switches them off again
 * (the default).  The converted bytes are the same with and without.  While statistics are on, a MIBAYER_FLAG_HIPGRAPH
 * context launches without graphs.  Arguments as above. */
int mibayer_set_stats (mibayer_ctx *ctx, int zones_x, int zones_y, uint32_t lo, uint32_t hi);
/* The zones (row-major; nzones = zones_x * zones_y as the frame was accepted with) of the frame most recently handed
 * back by mibayer_wait / mibayer_process_host; MIBAYER_ERR_EMPTY before the first such frame or when that frame was
 * accepted with statistics off, MIBAYER_ERR_ARG when nzones is not its zone count.  Call it from the thread that
 * retires the context's frames. */
int mibayer_frame_stats (mibayer_ctx *ctx, mibayer_stats_zone *out, int nzones);
/* ... of a pool: the grid of the frames mibayer_pool_submit accepts after it returns; the pool keeps the grid and the
 * zones with each frame, as it keeps the colour stage.  mibayer_pool_frame_stats returns those of the frame
 * mibayer_pool_wait handed back last, whichever shard converted it, also after a failover; a frame returned as lost
 * (MIBAYER_ERR_TIMEOUT) has none (MIBAYER_ERR_EMPTY). */
int mibayer_pool_set_stats (mibayer_pool *pool, int zones_x, int zones_y, uint32_t lo, uint32_t hi);
int mibayer_pool_frame_stats (mibayer_pool *pool, mibayer_stats_zone *out, int nzones);
/* Grey-world white balance from zones (pure host code, no device): all zones pooled per colour (both green sites into
 * G), m_k = (double) S_k / (double) N_k - black[k] (black may be NULL = 0).  Any N_k == 0 or m_k <= 0: gains = (1, 1, 1),
 * returns 0.  Else gains = (m_G / m_R, 1, m_G / m_B), each clamped to [1/16, 15.99], returns 1.  MIBAYER_ERR_ARG for a
 * NULL pointer, nzones < 1 or a pattern that is no mibayer_pattern. */
int mibayer_stats_grey_world (const mibayer_stats_zone *zones, int nzones, int pattern, const double black[3],
    double gains[3]);

/* ---- mosaic histogram (additive within version 5: a struct and the entry points of group `hist`) --------------- */

/* What auto exposure, auto levels and a clipping warning read: 256 bins per CFA site over a window of the MOSAIC, by a
 * read-only kernel.  Sample S, depth and site s as in group `stats` above.
 *   bin      S >> (depth - 8)
 *   window   (x0, y0, w, h): x0 and w even, w >= 2, h >= 1, x0 >= 0, y0 >= 0, x0 + w <= W, y0 + h <= H; (0, 0, 0, 0) is
 *            the whole frame, the last row of an odd height included.  Anything else: MIBAYER_ERR_ARG.  A window with
 *            more than 2^32 - 1 samples on one site: MIBAYER_ERR_GEOMETRY.
 * bin[s][b] = the number of samples of site s inside the window whose bin is b.  Columns >= W, stride padding and the
 * bits above `bits` never count.  Integers only: the result does not depend on the order of the kernel's atomics. */
#define MIBAYER_HIST_BINS 256
typedef struct mibayer_hist {           /* 4096 bytes */
  uint32_t bin[4][MIBAYER_HIST_BINS];   /* [site][bin] */
} mibayer_hist;

/* Device path: zeroes d_hist (nframes histograms, frame-major) on `hip_stream`, then ONE launch over the batch, frame f
 * read at d_src + f * src_frame_bytes as by mibayer_process_device.  Valid on every bayer2rgb context (8-bit, deep, MHC,
 * COLOUR, 24-bit, planar).  MIBAYER_ERR_ARG on an RGB2BAYER context, a window outside the rule above, d_src or d_hist not
 * a multiple of 4, nframes < 0; MIBAYER_ERR_GEOMETRY for a frame pitch as in mibayer_process_device.  Covered by
 * mibayer_sync when launched on the context's stream. */
int mibayer_hist_device (mibayer_ctx *ctx, const void *d_src, size_t src_frame_bytes, int nframes, int x0, int y0,
    int w, int h, mibayer_hist *d_hist, void *hip_stream);
/* Host path, as mibayer_set_stats / mibayer_frame_stats in every respect: on != 0, every frame accepted after this
 * returns also gets the histogram of that window, computed once on the slot's device copy of the mosaic behind the
 * (last band's) demosaic launch and downloaded with the frame into pinned memory of the slot; on = 0 switches it off
 * again (the default; the window is then ignored).  The converted bytes are the same with and without, a
 * MIBAYER_FLAG_HIPGRAPH context launches without graphs meanwhile, and statistics may be on as well.
 * mibayer_frame_hist: the histogram of the frame handed back last; MIBAYER_ERR_EMPTY before the first frame or when that
 * frame was accepted with histograms off. */
int mibayer_set_hist (mibayer_ctx *ctx, int on, int x0, int y0, int w, int h);
int mibayer_frame_hist (mibayer_ctx *ctx, mibayer_hist *out);
/* ... of a pool: window and histogram are kept with each frame like the zones; a frame redone on another shard brings
 * its own, a frame returned as lost has none (MIBAYER_ERR_EMPTY). */
int mibayer_pool_set_hist (mibayer_pool *pool, int on, int x0, int y0, int w, int h);
int mibayer_pool_frame_hist (mibayer_pool *pool, mibayer_hist *out);
/* Percentile bin (pure host code, no device).  colour 0 / 1 / 2 = R / G / B (both green sites pooled into G), 3 = all
 * four sites pooled; N = the pooled count.  N == 0: *bin = -1, returns 0.  Else rank r = max (1, (uint64) ceil (fraction
 * * (double) N)), *bin = the smallest b whose inclusive cumulative count is >= r, returns 1.  MIBAYER_ERR_ARG for a NULL
 * pointer, a pattern that is no mibayer_pattern, a colour outside 0 .. 3 or a fraction outside [0, 1] (NaN included). */
int mibayer_hist_percentile (const mibayer_hist *hist, int pattern, int colour, double fraction, int *bin);
/* Exposure factor from a histogram (pure host code, doubles, in exactly this order).  max = 2^depth - 1.  Per colour k:
 * b_k = its percentile bin at `fraction`, v_k = (b_k + 1) * 2^(depth - 8) - 1 (the top of that bin at native depth),
 * level_k = gains[k] * fmax (v_k - black[k], 0) / (max - black[k]); level = max_k level_k.  A colour without samples,
 * black[k] >= max or level <= 0: *exposure = 1, returns 0.  Else *exposure = clamp (target / level, 1/16, max_gain),
 * returns 1.  black NULL = 0, gains NULL = (1, 1, 1).  MIBAYER_ERR_ARG for a NULL hist or exposure, a bad pattern or
 * fraction, depth outside {8, 10, 12, 14, 16}, target outside (0, 1] or max_gain outside [1, 15.99]. */
int mibayer_hist_exposure (const mibayer_hist *hist, int pattern, int depth, const double black[3],
    const double gains[3], double fraction, double target, double max_gain, double *exposure);

/* ---- mosaic focus statistics (additive within version 5: a struct and the entry points of group `focus`) -------- */

/* The third measurement of a camera loop, next to the zones (white balance) and the histogram (exposure): a sharpness
 * measure per zone and CFA site of the MOSAIC, by a read-only kernel -- what auto focus, focus peaking and a lens set-up
 * read.  Sample S(x, y), depth, max = 2^depth - 1, site s = 2 (y & 1) + (x & 1), masking and byte order exactly as in
 * group `stats`, and so is the zone grid: zones_x x zones_y, each 1 .. 64, zones_x <= W/2, zones_y <= H/2, cells of
 * cw = 2 ceil ((W/2) / zones_x) by ch = 2 ceil ((H/2) / zones_y).  A sample belongs to the zone of its OWN (x, y) -- its
 * neighbours may lie in the adjacent zone --, the last row of an odd height has a zone, trailing zones may be empty and
 * are then all zero.
 *   responses  same-site second differences: rh = 2 S(x, y) - S(x - 2, y) - S(x + 2, y), defined only for 2 <= x <= W - 3,
 *              and rv = 2 S(x, y) - S(x, y - 2) - S(x, y + 2), defined only for 2 <= y <= H - 3.  Nothing is reflected or
 *              substituted: a response whose neighbour is off the frame does not exist (W = 4 has no rh, H = 3 or 4 no
 *              rv: the zones are then zero in that direction, which is no error).  Columns >= W, stride padding and the
 *              bits above `bits` never count.
 *   coring     a defined response contributes when |r| >= thr, thr in 0 .. 2 max (anything else: MIBAYER_ERR_ARG); with
 *              thr = 0 every defined response contributes, zeros included.
 * Integers only: the result does not depend on the order of the kernel's atomic additions.  Over a flat field of
 * independent noise of standard deviation sigma the mean response is sigma sqrt (12 / pi). */
typedef struct mibayer_focus_zone {     /* 96 bytes */
  uint64_t h[4];                /* sum of |rh| over the contributing samples of site s in the zone */
  uint64_t v[4];                /* likewise |rv| */
  uint32_t nh[4];               /* number of contributing rh */
  uint32_t nv[4];               /* number of contributing rv */
} mibayer_focus_zone;

/* Device path: zeroes d_focus (nframes * zones_y * zones_x zones, frame-major, then row-major) on `hip_stream`, then ONE
 * launch over the batch, frame f read at d_src + f * src_frame_bytes as by mibayer_process_device.  Valid on every
 * bayer2rgb context (8-bit, deep, MHC, COLOUR, 24-bit, planar).  Errors as mibayer_stats_device: MIBAYER_ERR_ARG on an
 * RGB2BAYER context, a grid outside the rule, thr > 2 max, d_src not a multiple of 4 or d_focus not a multiple of 8;
 * MIBAYER_ERR_GEOMETRY for a frame pitch as in mibayer_process_device.  Covered by mibayer_sync when launched on the
 * context's stream. */
int mibayer_focus_device (mibayer_ctx *ctx, const void *d_src, size_t src_frame_bytes, int nframes, int zones_x,
    int zones_y, uint32_t thr, mibayer_focus_zone *d_focus, void *hip_stream);
/* Host path, as mibayer_set_stats / mibayer_frame_stats in every respect: every frame accepted after this returns also
 * gets its focus zones, computed ONCE on the slot's device mosaic -- the one the demosaic reads, behind the defect, noise
 * reduction and shading passes; behind the last band of a banded frame -- and downloaded behind the frame into the slot's
 * pinned statistics buffer (zones, histogram, focus zones).  (0, 0) switches the measurement off again (the default:
 * nothing new is then called or allocated).  Converted bytes, zones and histograms are the same with and without; a
 * MIBAYER_FLAG_HIPGRAPH context launches without graphs meanwhile.  mibayer_frame_focus: the zones of the frame handed
 * back last; MIBAYER_ERR_EMPTY before the first frame or when that frame was accepted with focus off, MIBAYER_ERR_ARG
 * when nzones is not its zone count. */
int mibayer_set_focus (mibayer_ctx *ctx, int zones_x, int zones_y, uint32_t thr);
int mibayer_frame_focus (mibayer_ctx *ctx, mibayer_focus_zone *out, int nzones);
/* ... of a pool: grid, threshold and zones are kept with each frame like the zones and the histogram; a frame redone on
 * another shard brings its own, a frame returned as lost has none (MIBAYER_ERR_EMPTY). */
int mibayer_pool_set_focus (mibayer_pool *pool, int zones_x, int zones_y, uint32_t thr);
int mibayer_pool_frame_focus (mibayer_pool *pool, mibayer_focus_zone *out, int nzones);
/* Focus score from zones (pure host code, doubles, in exactly this order, no fused multiply-add).  colour 0 / 1 / 2 =
 * R / G / B (both green sites pooled), 3 = all four sites; weights NULL = 1, or nzones doubles, each finite and >= 0.
 * Per zone z over the sites s of the colour: A_z = (double) (sum_s h[s] + sum_s v[s]), N_z = (double) (sum_s nh[s] +
 * sum_s nv[s]), the site sums taken in uint64 first; A = sum_z w_z A_z, N = sum_z w_z N_z in zone order.  N not > 0:
 * *score = 0, returns 0.  Else *score = A / N -- the mean absolute response at native depth --, returns 1.
 * MIBAYER_ERR_ARG for a NULL zones or score, nzones < 1, a pattern that is no mibayer_pattern, a colour outside 0 .. 3
 * or a weight that is negative or not finite. */
int mibayer_focus_score (const mibayer_focus_zone *zones, int nzones, int pattern, int colour, const double *weights,
    double *score);

/* ---- lens shading correction (additive within version 5: a struct and the entry points of group `shading`) ------ */

/* Vignetting and colour shading: a gain per CFA site that varies smoothly over the frame, applied to the MOSAIC by a
 * pointwise kernel before the demosaic, the statistics and the histogram read it.  Integers only, bit-exact.
 *   sample   S, depth, max = 2^depth - 1 and site s = 2 (y & 1) + (x & 1) exactly as in group `stats`: the byte of an
 *            8-bit mosaic, or the 16-bit word in the context's byte order masked to `bits`
 *   grid     cells of cw = 1 << kx by ch = 1 << ky pixels, kx and ky in 2 .. 8; nodes nx = ((W - 1) >> kx) + 2,
 *            ny = ((H - 1) >> ky) + 2; more than 129 nodes in a direction: MIBAYER_ERR_ARG.  The table is
 *            uint16_t g[4][ny][nx], site-major, Q12 (4096 = 1.0), every entry in 0 .. 32767 (above: MIBAYER_ERR_ARG)
 *   gain     at (x, y), with g = the plane of the pixel's site: i = x >> kx, fx = x & (cw - 1), j = y >> ky,
 *            fy = y & (ch - 1),
 *              G = ((g[j][i] (cw - fx) + g[j][i+1] fx) (ch - fy) + (g[j+1][i] (cw - fx) + g[j+1][i+1] fx) fy
 *                   + (1 << (kx + ky - 1))) >> (kx + ky)                  exact in uint32: 32767 * 2^16 < 2^32
 *   apply    black[4] per site, each <= max (else MIBAYER_ERR_ARG):  d = S - black[s]  (signed),
 *              out = clamp (black[s] + ((d G + 2048) >> 12), 0, max)      arithmetic shift; d G + 2048 fits int32
 *            a deep sample is written as the 16-bit word in the source's byte order with the bits above `bits` zero.
 *            Only the first W samples of a row are written: the stride padding of an out-of-place destination keeps
 *            what it held.
 * An all-4096 table is the identity on the masked samples, whatever the black levels. */
typedef struct mibayer_shading {
  uint32_t struct_size;         /* = sizeof (mibayer_shading) */
  int32_t cell_log2_x;          /* kx */
  int32_t cell_log2_y;          /* ky */
  uint32_t black[4];            /* per site, at native depth */
  const uint16_t *table;        /* host memory, 4 * ny * nx entries; copied */
} mibayer_shading;
#define MIBAYER_SHADING_MAX_NODES 129   /* per direction */

/* nodes of a width x height frame under cells of (1 << kx) x (1 << ky) (pure host code).  MIBAYER_ERR_ARG for a NULL
 * pointer, width or height < 1, kx or ky outside 2 .. 8, or more than MIBAYER_SHADING_MAX_NODES in a direction. */
int mibayer_shading_nodes (int width, int height, int kx, int ky, int *nx, int *ny);
/* Sets the table of a context (NULL: off, the default).  Valid on every bayer2rgb context (8-bit, deep, MHC, COLOUR,
 * 24-bit, planar); MIBAYER_ERR_ARG on an RGB2BAYER context, a bad struct_size, a NULL table and on values outside the
 * rules above.  The table is copied into device memory of the context before the call returns.  It applies to the
 * frames accepted (mibayer_submit / mibayer_process_host) and the mibayer_shade_device calls made after it returns;
 * frames already accepted keep the table they were accepted with.  May be called between frames, from any thread.
 * HOST PATH: while a table is set, every accepted frame is shaded in place on the device copy of the mosaic that its
 * ring slot holds, each row exactly once (band by band when the frame is launched in bands), before anything else
 * reads it: the demosaic, the statistics and the histogram of the frame see corrected samples.  While a table is set a
 * MIBAYER_FLAG_HIPGRAPH context launches without graphs.  With no table the bytes are those of the same context
 * before this entry point existed.  mibayer_process_device[_list] never shades: its source is const.
 * mibayer_get_shading: out->table = NULL and returns MIBAYER_ERR_EMPTY when none is set; else the parameters, with
 * out->table pointing at the context's host copy (valid until the next mibayer_set_shading / mibayer_destroy). */
int mibayer_set_shading (mibayer_ctx *ctx, const mibayer_shading *shading);
int mibayer_get_shading (const mibayer_ctx *ctx, mibayer_shading *out);
/* Device path: ONE launch shading `nframes` mosaics with the table set before, frame f read at d_src + f *
 * src_frame_bytes (rows of cfg.src_stride bytes) and written at d_dst + f * dst_frame_bytes in the same layout;
 * d_dst == d_src is allowed: every sample is read and written by the same lane.  In place the two pitches must be
 * equal (nframes > 1 with d_dst == d_src and dst_frame_bytes != src_frame_bytes: MIBAYER_ERR_GEOMETRY); a destination
 * that overlaps the source in any other way is undefined.  Errors follow
 * mibayer_stats_device: MIBAYER_ERR_ARG on an RGB2BAYER context, a NULL pointer, nframes < 0, a pointer that is not a
 * multiple of 4; MIBAYER_ERR_GEOMETRY for a frame pitch (of either side) as in mibayer_process_device;
 * MIBAYER_ERR_EMPTY when no table is set.  Covered by mibayer_sync when launched on the context's stream. */
int mibayer_shade_device (mibayer_ctx *ctx, const void *d_src, size_t src_frame_bytes, void *d_dst,
    size_t dst_frame_bytes, int nframes, void *hip_stream);
/* ... of a pool: the table of the frames mibayer_pool_submit accepts after it returns (NULL: off).  The pool keeps the
 * table with each frame, like the colour stage, and hands it to a shard's context together with the frame: a frame
 * converted again on another shard after a failover is shaded there, from its host copy, with the table it was
 * submitted with.  Call it from the thread that calls mibayer_pool_submit. */
int mibayer_pool_set_shading (mibayer_pool *pool, const mibayer_shading *shading);
/* A table from the zone statistics of a FLAT FIELD (pure host code, doubles, in exactly this order; no fused
 * multiply-add).  zones: zones_y x zones_x of a width x height frame (mibayer_stats_device / mibayer_frame_stats);
 * zcw, zch = the pixels and rows of a zone as in group `stats`; ux = ceil (W / zcw), uy = ceil (H / zch) zones per
 * direction hold pixels, the others are ignored.  Centre of zone column a: cx[a] = (a zcw + min ((a + 1) zcw, W)) * 0.5,
 * of zone row b: cy[b] likewise with zch and H.  Per site s:
 *   1. m[b][a] = (double) sum[s] / (double) count[s] - (double) black[s] for a zone with count[s] > 0; an empty zone
 *      takes m of the non-empty zone (a', b') with the smallest (a' - a)^2 + (b' - b)^2, the first in row-major order
 *      among equals.  No non-empty zone: all of table_out = 4096, returns 0.
 *   2. node (j, i) lies at px = (double) (i << kx), py = (double) (j << ky).  Along x: px <= cx[0] (or ux == 1): a = 0,
 *      tx = 0; px >= cx[ux-1]: a = ux - 1, tx = 0; else a = the largest index with cx[a] <= px and
 *      tx = (px - cx[a]) / (cx[a+1] - cx[a]); a1 = min (a + 1, ux - 1).  Along y alike: b, ty, b1.
 *        top = m[b][a] + (m[b][a1] - m[b][a]) * tx,  bot = m[b1][a] + (m[b1][a1] - m[b1][a]) * tx,
 *        v[j][i] = top + (bot - top) * ty
 *      Any v that is not > 0: all of table_out = 4096, returns 0.
 *   3. vmax = the largest v of the site; gain = vmax / v[j][i], clamped to [1, max_gain];
 *      g[s][j][i] = (uint16_t) floor (gain * 4096 + 0.5).
 * Returns 1.  black NULL = 0.  MIBAYER_ERR_ARG for a NULL zones or table_out, a zone grid outside the rule of group
 * `stats`, width < 2 or odd, height < 1, a grid as in mibayer_shading_nodes, or max_gain outside [1, 7.99] (NaN
 * included). */
int mibayer_stats_shading (const mibayer_stats_zone *zones, int zones_x, int zones_y, int width, int height,
    const uint32_t black[4], int kx, int ky, double max_gain, uint16_t *table_out);

/* ---- defective pixel correction (additive within version 5: a struct and the entry points of group `dpc`) -------- */

/* Stuck and dead samples, corrected on the MOSAIC before the shading pass, the statistics, the histogram and the
 * demosaic read it.  Integers only, bit-exact.
 *   sample   S at (x, y), depth, max = 2^depth - 1 and site exactly as in group `stats`; a deep sample is masked and
 *            byte-swapped on read as in group `shading`
 *   neighbours  the eight samples of the same site at (x + dx, y + dy), dx, dy in {-2, 0, 2}, not both 0.  A coordinate
 *            off the frame is replaced by the one on the other side of the pixel: x - 2 < 0 -> x + 2, x + 2 >= W ->
 *            x - 2, and the same for y with H.  This keeps the site and needs W >= 4 (every context) and H >= 4 (a
 *            context with H = 3: MIBAYER_ERR_GEOMETRY).  hi = the largest, lo = the smallest of the eight
 *   detect   hot and cold thresholds at native depth, -1 = off, else 0 .. max:
 *              hot:  S > hi + hot            cold:  S + cold < lo
 *   replace  four pairs, in this order:  H (x-2, y), (x+2, y)   V (x, y-2), (x, y+2)   D1 (x-2, y-2), (x+2, y+2)
 *            D2 (x+2, y-2), (x-2, y+2).  g = |a - b| per pair; the pair with the smallest g wins, the first in that
 *            order among equals; R = (a + b + 1) >> 1
 *   out      R if the sample is hot, cold or listed, else S.  Neighbours are always those of the SOURCE, never
 *            corrected values: out is a pure function of the source frame, which is why the pass cannot run in place.
 *            Two listed defects of one site two pixels apart therefore see each other (open item: excluding listed
 *            neighbours from the pairs).  A deep sample is written as the 16-bit word in the source's byte order with
 *            the bits above `bits` zero.  Only the first W samples of a row are written: the stride padding of the
 *            destination keeps what it held.
 *   list     up to MIBAYER_DPC_MAX_DEFECTS (x, y) pairs, uint32_t xy[2 n], in any order; the library keeps a copy sorted
 *            by (y, x) with duplicates dropped.  A coordinate outside the frame: MIBAYER_ERR_ARG.
 * Both thresholds off and an empty list is the identity on the masked samples. */
typedef struct mibayer_dpc {
  uint32_t struct_size;         /* = sizeof (mibayer_dpc) */
  int32_t hot;                  /* -1 = off, else 0 .. max */
  int32_t cold;                 /* likewise */
  uint32_t ndefects;            /* <= MIBAYER_DPC_MAX_DEFECTS */
  const uint32_t *defects;      /* host memory, x0 y0 x1 y1 ...; copied; may be NULL when ndefects = 0 */
} mibayer_dpc;
#define MIBAYER_DPC_MAX_DEFECTS 65536

/* Sets the correction of a context (NULL: off, the default).  Valid on every bayer2rgb context; MIBAYER_ERR_ARG on an
 * RGB2BAYER context, a bad struct_size, a threshold outside -1 .. max, ndefects above the maximum, a NULL list with
 * ndefects > 0 and a coordinate outside the frame; MIBAYER_ERR_GEOMETRY on a context with H < 4.  The list is copied
 * into device memory of the context before the call returns.  It applies to the frames accepted (mibayer_submit /
 * mibayer_process_host) and the mibayer_dpc_device calls made after it returns; frames already accepted keep the
 * parameters they were accepted with.  May be called between frames, from any thread.
 * HOST PATH: while the correction is set, a ring slot holds a second device mosaic (allocated when first needed, freed
 * with the slot): the upload lands there and the pass writes the slot's mosaic, each row exactly once (band by band
 * when the frame is launched in bands, two rows behind the upload), before the shading pass -- which then runs in
 * place on corrected samples -- and before anything else reads it.  While it is set a MIBAYER_FLAG_HIPGRAPH context
 * launches without graphs.  With the correction off nothing new is called or allocated and the bytes are those of the
 * same context before this entry point existed.  mibayer_process_device[_list] never corrects.
 * mibayer_get_dpc: MIBAYER_ERR_EMPTY when off; else the parameters, with out->defects pointing at the context's sorted,
 * de-duplicated copy (valid until the next mibayer_set_dpc / mibayer_destroy) and out->ndefects its length. */
int mibayer_set_dpc (mibayer_ctx *ctx, const mibayer_dpc *dpc);
int mibayer_get_dpc (const mibayer_ctx *ctx, mibayer_dpc *out);
/* Device path: one batch, `nframes` mosaics corrected with the parameters set before, frame f read at d_src + f *
 * src_frame_bytes (rows of cfg.src_stride bytes) and written at d_dst + f * dst_frame_bytes in the same layout.  Out of
 * place only: d_dst == d_src is MIBAYER_ERR_ARG, and any other overlap of source and destination is undefined.  The
 * other errors are those of mibayer_shade_device; MIBAYER_ERR_EMPTY when the correction is off.  Covered by
 * mibayer_sync when launched on the context's stream. */
int mibayer_dpc_device (mibayer_ctx *ctx, const void *d_src, size_t src_frame_bytes, void *d_dst,
    size_t dst_frame_bytes, int nframes, void *hip_stream);
/* ... of a pool: the correction of the frames mibayer_pool_submit accepts after it returns (NULL: off), kept with each
 * frame and handed to a shard's context together with the frame, like the shading table.  Call it from the thread that
 * calls mibayer_pool_submit. */
int mibayer_pool_set_dpc (mibayer_pool *pool, const mibayer_dpc *dpc);

/* ---- noise reduction (additive within version 5: a struct and the entry points of group `nr`) --------------------- */

/* Spatial noise reduction on the MOSAIC, behind the defect pass and before the shading pass, the statistics, the
 * histogram and the demosaic read it: the shading gain, the colour matrix and the tone curve amplify what is left, and the
 * demosaic spreads it over a coloured neighbourhood.  Integers only, bit-exact.
 *   sample   S at (x, y); depth, max = 2^depth - 1, site, masking and byte order on read and write exactly as in group
 *            `dpc`
 *   window   the 24 neighbours of the same site at (x + dx, y + dy), dx, dy in {-4, -2, 0, 2, 4}, not both 0
 *   border   a coordinate off the frame is reflected about the edge sample: x < 0 -> -x, x >= W -> 2 (W - 1) - x, and
 *            the same for y with H (numpy.pad mode "reflect").  This keeps the site and, unlike the defect pass's rule,
 *            replaces a row by one that depends on the row index only.  It needs W >= 6 and H >= 5: a smaller context
 *            is MIBAYER_ERR_GEOMETRY
 *   threshold  a curve of MIBAYER_NR_NODES = 17 nodes curve[0 .. 16] over the sample's level, each 0 .. T_MAX, T_MAX = 255
 *            for an 8-bit mosaic and min (max, 2047) for a deep one.  With sh = depth - 4, s = 1 << sh, k = S >> sh and
 *            f = S & (s - 1):   t = (curve[k] (s - f) + curve[k + 1] f + (s >> 1)) >> sh
 *   filter   a neighbour n is included when |n - S| <= t.  P = the sum of n - S over the included n > S, N = the sum of
 *            S - n over the included n < S (both <= 24 T_MAX < 2^16), cnt = 1 + the number included (1 .. 25),
 *            v = P - N, q = (2 |v| + cnt) / (2 cnt) rounded down, out = S + q where v >= 0, S - q where v < 0: the mean of
 *            the included samples and the centre, rounded half away from S.  It lies between the smallest and the
 *            largest of them: nothing is clamped
 *   out      a pure function of the SOURCE frame -- neighbours are never filtered values -- which is why the pass cannot
 *            run in place.  Written as in group `dpc`: only the first W samples of a row, the stride padding of the
 *            destination keeps what it held.
 * An all-zero curve is the identity on the masked samples. */
#define MIBAYER_NR_NODES 17
typedef struct mibayer_nr {
  uint32_t struct_size;         /* = sizeof (mibayer_nr) */
  uint16_t curve[17];           /* thresholds at the levels i << (depth - 4), each 0 .. T_MAX */
  uint16_t reserved;            /* padding; ignored */
} mibayer_nr;

/* Sets the curve of a context (NULL: off, the default).  Valid on every bayer2rgb context; MIBAYER_ERR_ARG on an
 * RGB2BAYER context, a bad struct_size and a node above T_MAX; MIBAYER_ERR_GEOMETRY on a context with W < 6 or H < 5.
 * It applies to the frames accepted (mibayer_submit / mibayer_process_host) and the mibayer_nr_device calls made after
 * it returns; frames already accepted keep the curve they were accepted with.  May be called between frames, from any
 * thread.
 * HOST PATH: while a curve is set, a ring slot holds one more device mosaic (allocated when first needed, freed with
 * the slot; three with the defect pass set too): the pass reads what the upload -- or the defect pass -- wrote and writes
 * the slot's mosaic, each row exactly once (band by band when the frame is launched in bands, four rows behind the rows
 * the defect pass has finished), before the shading pass -- which then runs in place on denoised samples -- and before
 * anything else reads it.  While it is set a MIBAYER_FLAG_HIPGRAPH context launches without graphs.  With the curve off
 * nothing new is called or allocated and the bytes are those of the same context before this entry point existed.
 * mibayer_process_device[_list] never denoises.
 * mibayer_get_nr: MIBAYER_ERR_EMPTY when off; else the curve. */
int mibayer_set_nr (mibayer_ctx *ctx, const mibayer_nr *nr);
int mibayer_get_nr (const mibayer_ctx *ctx, mibayer_nr *out);
/* Device path: one batch, `nframes` mosaics denoised with the curve set before, frame f read at d_src + f *
 * src_frame_bytes (rows of cfg.src_stride bytes) and written at d_dst + f * dst_frame_bytes in the same layout.  Out of
 * place only: d_dst == d_src is MIBAYER_ERR_ARG, and any other overlap of source and destination is undefined.  The
 * other errors are those of mibayer_dpc_device; MIBAYER_ERR_EMPTY when the curve is off.  Covered by mibayer_sync when
 * launched on the context's stream. */
int mibayer_nr_device (mibayer_ctx *ctx, const void *d_src, size_t src_frame_bytes, void *d_dst,
    size_t dst_frame_bytes, int nframes, void *hip_stream);
/* ... of a pool: the curve of the frames mibayer_pool_submit accepts after it returns (NULL: off), kept with each frame
 * and handed to a shard's context together with the frame, like the defect pass's parameters.  Call it from the thread
 * that calls mibayer_pool_submit. */
int mibayer_pool_set_nr (mibayer_pool *pool, const mibayer_nr *nr);
/* A curve from a sensor's noise model, host arithmetic in IEEE doubles: node i sits at the level v = i << (depth - 4)
 * and gets t = floor (strength * sqrt (read_noise^2 + shot_noise * max (v - black, 0)) + 0.5), clamped to T_MAX.
 * `bits`: 8, 10, 12, 14 or 16; black, read_noise (DN at native depth), shot_noise (DN of variance per DN of signal) and
 * strength (thresholds per standard deviation) >= 0 and finite, else MIBAYER_ERR_ARG, as are a NULL `out` and any other
 * depth.  Fills out->struct_size. */
int mibayer_nr_curve (int bits, double black, double read_noise, double shot_noise, double strength, mibayer_nr *out);

/* ---- global ------------------------------------------------------------- */

int mibayer_abi_version (void);
/* PCI bus id ("0000:c1:00.0", NUL-terminated; len >= 13) of a HIP ordinal: the physical identity of the card a
 * context, pool shard or bench rank runs on (v5). */
int mibayer_device_pci_bus_id (int device, char *out, size_t len);
/* 1 = this library was built with -DMIBAYER_LAB (`make lab`): the experiment
 * kernel arms and the tuning environment variables of DESIGN.md are compiled in.
 * 0 = the product build: the three production tile shapes with their store-policy
 * twins, and no tuning environment. */
int mibayer_is_lab_build (void);
/* number of HIP devices, 0 if none (never negative) */
int mibayer_device_count (void);
const char *mibayer_strerror (int status);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char *mibayer_last_hip_error (void);

/* ---- per-stream context (created in set_caps, destroyed in stop/finalize) -- */

/* Validates cfg, selects the device, creates the compute and copy streams and
 * the device-side frame ring.  Replaces the per-frame g_malloc'ed scratch of
 * the reference (:429) with state that lives as long as the caps do. */
int mibayer_create (const mibayer_cfg *cfg, mibayer_ctx **out);
void mibayer_destroy (mibayer_ctx *ctx);
/* the configuration with every default resolved */
int mibayer_get_cfg (const mibayer_ctx *ctx, mibayer_cfg *out);

/* ---- host-memory frame path (what the GStreamer element calls) ------------ */

/* Synchronous drop-in for gst_bayer2rgb_process (:475-477): `src` holds
 * src_stride*height bytes, `dst` receives dst_stride*height bytes (only the
 * first 4*width bytes of each row are written); returns when dst is complete.
 * H2D, kernel and D2H run on the context's streams.  src/dst may be pageable
 * or pinned (mibayer_host_alloc) memory. */
int mibayer_process_host (mibayer_ctx *ctx, const uint8_t *src, uint8_t *dst);

/* Asynchronous form: up to cfg.inflight frames between submit and wait.
 * Frames complete in submission order; `tag` is handed back by wait.
 * src/dst must stay valid until the matching wait returns. */
int mibayer_submit (mibayer_ctx *ctx, const uint8_t *src, uint8_t *dst,
    void *tag);
int mibayer_wait (mibayer_ctx *ctx, void **tag);
int mibayer_pending (const mibayer_ctx *ctx);
/* Deadline, in milliseconds, of every host-side wait for the device on behalf of
 * this context (mibayer_wait, mibayer_process_host, mibayer_sync, mibayer_destroy):
 * a GPU that has stopped answering completes nothing, and the reference's
 * streaming thread must not hang on it (cf. gst/debugutils/gstwatchdog.c:21-123).
 * Default 10000 (also MIBAYER_WAIT_TIMEOUT_MS); 0 = wait for ever; < 0 = default.
 * A wait that runs into the deadline returns MIBAYER_ERR_TIMEOUT and leaves the
 * frame where it is -- its buffers still belong to the device.  The deadline also
 * bounds mibayer_sync() after device-resident launches: a device that is shared
 * with long-running foreign kernels needs a longer one. */
int mibayer_set_wait_timeout (mibayer_ctx *ctx, int ms);
/* How a host-side wait spends its time.  The completion event is polled: a tight
 * loop for `spin_us` microseconds, then naps that double from 20 us to 250 us.
 * spin_us < 0 (the default; also MIBAYER_WAIT_SPIN_US) = automatic: spin (up to
 * 2 ms) only while the frame waited for is the only one in flight -- the
 * synchronous 1-in/1-out use, where a nap's wake-up latency comes straight off
 * the frame rate -- and nap from the start when other frames are queued behind
 * it (they keep the device busy while the thread sleeps): a few wake-ups per
 * frame instead of a core per streaming thread. */
int mibayer_set_wait_spin (mibayer_ctx *ctx, int spin_us);
/* Host CPU the context has cost its callers so far: calls and CPU time
 * (CLOCK_THREAD_CPUTIME_ID of the calling threads) inside submit and inside the
 * waits, the waits' wall time, hipEventQuery polls and naps. */
typedef struct mibayer_host_stats {
  uint64_t submits;
  uint64_t waits;
  uint64_t polls;
  uint64_t naps;
  double submit_cpu_ms;
  double wait_cpu_ms;
  double wait_wall_ms;
} mibayer_host_stats;
int mibayer_get_host_stats (const mibayer_ctx *ctx, mibayer_host_stats *out);

/* ---- multi-GPU frame sharding (host path) ------------------------------------ */

/* Frames are independent (the reference keeps no state between frames,
 * gstbayer2rgb.c:387-451), so a stream is sharded round-robin over GPUs with no
 * collective: frame g goes to shard g % ndevices, every shard is a mibayer_ctx
 * with its own device ring and (optionally) graphs, and results are handed back
 * in submission order.  By default the calling thread drives all shards -- with
 * pinned buffers every call below only enqueues work -- and a shard that sees
 * pageable buffers gets a helper thread (queueing a 4K frame from pinned buffers
 * costs the caller 14-80 us of CPU, from pageable ones 200-300 us: the runtime's
 * staging copy).  One thread saturates at ~11 k frames/s, what eight PCIe links
 * carry at 4K: pools over six or more DISTINCT GPUs give every shard its own
 * submit thread from the start; MIBAYER_POOL_THREADS=1 / 0 forces that on / off.  When the devices span more than
 * one NUMA node, a frame goes to the live shard next to its 4-byte-per-pixel
 * buffer as long as that keeps the rotation balanced (MIBAYER_POOL_NUMA=0:
 * strictly g % ndevices).  Ordinals may repeat (N logical shards on one GPU). */
#define MIBAYER_MAX_SHARDS 16
typedef struct mibayer_pool_cfg {
  uint32_t struct_size;         /* = sizeof (mibayer_pool_cfg)                  */
  mibayer_cfg stream;           /* geometry, order, layout, inflight PER SHARD,
                                   flags; .device is ignored                    */
  int32_t ndevices;             /* 1 .. MIBAYER_MAX_SHARDS                      */
  int32_t devices[MIBAYER_MAX_SHARDS];  /* HIP ordinals                         */
} mibayer_pool_cfg;

int mibayer_pool_create (const mibayer_pool_cfg *cfg, mibayer_pool **out);
void mibayer_pool_destroy (mibayer_pool *pool);
/* total frames that may be in flight = live devices * stream.inflight (shrinks
 * when a device is dropped, see below) */
int mibayer_pool_capacity (const mibayer_pool *pool);
int mibayer_pool_pending (const mibayer_pool *pool);
/* MIBAYER_ERR_BUSY when the shard whose turn it is has its share of frames in
 * flight: call mibayer_pool_wait() first.  Frames whose src or dst is pageable
 * memory are converted by a helper thread of their shard (the copies block the
 * thread that issues them), so this call only queues either way. */
int mibayer_pool_submit (mibayer_pool *pool, const uint8_t *src, uint8_t *dst,
    void *tag);
/* oldest frame first */
int mibayer_pool_wait (mibayer_pool *pool, void **tag);

/* Failure handling.  The reference's only reaction to a failure on this path is
 * "warn and carry on" (gstbayer2rgb.c:484-486).  A device that reports a HIP
 * error (or runs out of memory) is dropped from the rotation, the frames it
 * still held are converted again on the surviving devices -- same bytes, same
 * order -- and the stream carries on; submit / wait return MIBAYER_ERR_HIP only
 * when no device is left.  mibayer_pool_take_failure() returns the number of
 * devices dropped since the last call (0 = none) with the ordinal of the latest
 * one, the number of devices left and a one-line description. */
int mibayer_pool_alive (const mibayer_pool *pool);
int mibayer_pool_take_failure (mibayer_pool *pool, int *device, int *alive,
    char *msg, size_t msg_len);
/* Failure drill: shard `shard` (index into devices[]) reports a device error
 * once it has completed `after_frames` more frames; negative = cancel.  The
 * environment variable MIBAYER_INJECT_FAULT="shard:frames[,shard:frames]" does
 * the same at mibayer_pool_create(). */
int mibayer_pool_inject_fault (mibayer_pool *pool, int shard,
    long long after_frames);
/* The wait deadline of every shard (mibayer_set_wait_timeout): a device that
 * does not complete a frame within `ms` milliseconds is dropped from the rotation
 * like one that reported an error, and is never waited for again. */
int mibayer_pool_set_wait_timeout (mibayer_pool *pool, int ms);
int mibayer_pool_set_wait_spin (mibayer_pool *pool, int spin_us);
/* sum over the shards */
int mibayer_pool_get_host_stats (const mibayer_pool *pool, mibayer_host_stats *out);
/* Frames that were IN FLIGHT on a device when it ran into the wait deadline are
 * not converted again behind the device's back: the device may only be slow, its
 * queued copies may still read the frame's source and write its destination
 * later.  mibayer_pool_wait() hands such a frame back -- in order, with its tag --
 * with MIBAYER_ERR_TIMEOUT: the frame is LOST (drop it), the stream carries on on
 * the remaining devices (mibayer_pool_alive() == 0: it has failed), and both
 * buffers of the frame stay the device's: do not free, unmap or reuse them until
 * mibayer_pool_reclaim() hands the tag back -- it does once the device has caught
 * up with everything it had queued (non-blocking; MIBAYER_ERR_EMPTY = none ready).
 * mibayer_pool_lost() = lost frames not reclaimed yet.  Buffers still lost when
 * the pool is destroyed must be leaked.  Frames the dropped device had not been
 * given yet are converted on the others as after a device error. */
int mibayer_pool_reclaim (mibayer_pool *pool, void **tag);
int mibayer_pool_lost (const mibayer_pool *pool);
/* Stall drill: the compute queue of shard `shard` is occupied for `ms`
 * milliseconds (1 .. 5000) by a kernel that only waits -- a device that has
 * stopped answering, as far as the host can tell. */
int mibayer_pool_inject_stall (mibayer_pool *pool, int shard, int ms);

/* ---- device-resident batch path (roofline runs, GPU-side consumers) -------- */

/* Enqueues ONE kernel launch converting `nframes` frames that already live in
 * device memory: frame f is read at d_src + f*src_frame_bytes and written at
 * d_dst + f*dst_frame_bytes.  `hip_stream` is the hipStream_t to launch on,
 * used as given (NULL is HIP's null stream); pass mibayer_ctx_stream() for the
 * context's own compute stream.  Returns after the launch is enqueued. */
int mibayer_process_device (mibayer_ctx *ctx, const void *d_src,
    size_t src_frame_bytes, void *d_dst, size_t dst_frame_bytes, int nframes,
    void *hip_stream);
/* The same for frames that are SEPARATE device allocations (one GstBuffer each):
 * frame f is read at d_srcs[f] and written at d_dsts[f]; up to 16 frames go into
 * one kernel launch (more are split).  For device-resident pipelines, where a
 * launch per 4K frame costs as much as the kernel runs (gst/gstmihipelements.c,
 * hipbayer2rgb batch=N). */
int mibayer_process_device_list (mibayer_ctx *ctx, const void *const *d_srcs,
    void *const *d_dsts, int nframes, void *hip_stream);
/* the context's compute stream (a hipStream_t), created non-blocking */
void *mibayer_ctx_stream (mibayer_ctx *ctx);
/* Frame queues (v5): MIBAYER_FRAME_QUEUES compute streams per DEVICE, each on a hardware queue of its own, shared by
 * the contexts of the device, created on first use (NULL: k out of range, or no stream could be made) and kept for the
 * life of the process (destroying such a stream hangs intermittently in ROCm 7.2).  A launch over
 * ONE frame is a single round of workgroups -- ramp-up, one burst of loads, one burst of stores, drain: 4K 9.4 us
 * against 6.5 us per frame inside a batch -- so a caller that converts frame after frame (one GstBuffer at a time) and
 * whose frames do not depend on each other deals them round-robin over the frame queues: the ramp-up of the next
 * frames overlaps the drain of frame n (4K: 54 % of HBM peak on one queue, 66-67 % on four; rgb2bayer 55 -> 77 %).
 * That is for launches WITHOUT per-frame dependencies on other queues: a frame that must wait for an event of its
 * producer's queue and is waited for by its consumer's pays more for the cross-queue dependencies than the overlap
 * gains (hipbayer2rgb from a device-resident source: 14.5 k fps with the frame queues, 36 k without -- the elements'
 * `overlap` property is therefore off by default).  Ordinary HIP streams share a small pool of hardware queues and serialise
 * behind each other again; these do not.  The queues are not ordered against each other or against
 * mibayer_ctx_stream(): order consumers with events (mibayer_dev_event_record / mibayer_dev_stream_wait_event) or with
 * mibayer_sync(), which covers every frame queue this context launched on.
 * One exception to "not ordered" (ADVICE r05): hipExtStreamCreateWithCUMask takes no flags, so these are BLOCKING
 * streams in the runtime's sense -- they synchronise implicitly with HIP's legacy NULL stream, in both directions,
 * unlike every other stream of this library (hipStreamNonBlocking), and unlike the plain non-blocking streams that
 * stand in for them when the CU-mask call fails.  A process that launches on the NULL stream (or on a framework's
 * "default stream" that is the NULL stream) serialises frame-queue launches against it: drive the frame queues from
 * processes whose other work is on explicit streams, as the elements and tools/single_frame_bench.py do. */
#define MIBAYER_FRAME_QUEUES 4
void *mibayer_ctx_frame_queue (mibayer_ctx *ctx, int k);
/* Waits (with the context's deadline) for what THIS context has in flight: its
 * pending host-path frames and the device-resident work queued through
 * mibayer_process_device[_list] / mibayer_fill_synthetic on mibayer_ctx_stream() and
 * mibayer_process_device[_list] on the frame queues (mibayer_ctx_frame_queue).
 * Work a caller put on that stream by other means (its own kernels, copies) is
 * NOT covered -- the queue may be shared with the other contexts of the device --
 * and neither is work on a caller-supplied stream: synchronise those yourself. */
int mibayer_sync (mibayer_ctx *ctx);

/* Times `reps` back-to-back launches of mibayer_process_device on the context's
 * compute stream with HIP events recorded on that stream (after `warmup` untimed
 * launches); writes the mean milliseconds per launch. */
int mibayer_time_device (mibayer_ctx *ctx, const void *d_src,
    size_t src_frame_bytes, void *d_dst, size_t dst_frame_bytes, int nframes,
    int warmup, int reps, float *ms_per_launch);

/* Measured launch-plan selection for the device-resident path.  MI355X boxes --
 * and allocations -- differ in which block->tile order streams best (DESIGN.md
 * "XCD map"): this call times the candidate plans on the caller's own buffers with
 * HIP events on the context's compute stream and keeps the fastest for every later
 * launch of this context THAT FALLS INTO THE SAME LAUNCH CLASS as the `nframes`-frame launches it timed (v5: launch
 * classes, below; a plan measured on 64-frame batches does not become the plan of one-frame launches).  Candidates: the three production tile shapes x {band 1,
 * one chunk per XCD, identity order}; for generic geometries whose output rows sit
 * off the 64-byte sector grid additionally x {streaming, write-back, hybrid}
 * stores, plus the shifted arm (every wave-store on a 128-byte boundary) in the two
 * narrow shapes.  A common time-based warm-up (>= 60 ms of launches), then five
 * interleaved rounds of a few launches per candidate; with more than nine
 * candidates only those within 6 % of the best of the first round stay in; the
 * MEDIAN round counts.  The kernel is idempotent, so d_dst holds the correct output
 * afterwards.  Synchronous.  `report` (may be NULL) receives a one-line summary. */
int mibayer_autotune (mibayer_ctx *ctx, const void *d_src,
    size_t src_frame_bytes, void *d_dst, size_t dst_frame_bytes, int nframes,
    char *report, size_t report_len);

/* The same over frames that are SEPARATE device allocations, timed through
 * mibayer_process_device_list (what a device-resident element holds: one GstBuffer
 * per frame). */
int mibayer_autotune_list (mibayer_ctx *ctx, const void *const *d_srcs,
    void *const *d_dsts, int nframes, char *report, size_t report_len);

/* Copies the launch plan chosen by mibayer_autotune() to another context of the
 * same width/height (e.g. the same camera geometry in another Bayer order). */
int mibayer_copy_plan (mibayer_ctx *dst, const mibayer_ctx *src);

/* The launch plan as a value: kernel variant id (1 .. mibayer_variant_count()-1),
 * block order (tile rows per XCD band: 1, N; 0 = identity; -1 = one chunk of the
 * batch per XCD; INT32_MIN = the variant's default) and the store alignment of the
 * shifted arm for generic geometries (0 = off, 64, 128).  Any out pointer may be
 * NULL.  Every plan is bit-exact; a plan only changes speed. */
int mibayer_get_plan (const mibayer_ctx *ctx, int *variant, int *band,
    int *align_stores);
int mibayer_set_plan (mibayer_ctx *ctx, int variant, int band, int align_stores);
/* Launch classes (v5).  A context keeps one plan per class of launch:
 *   batch class -- launches that keep every workgroup slot of the device busy for many rounds (the 64-frame batch);
 *   frame class -- launches of at most 4 rounds of workgroups (on 256 CUs: up to 33.5 Mpixel per launch = one 8K
 *                  frame, four 4K frames): what an element or the host path issues, one frame per launch.  Its default
 *                  shape is the production shape whose grid needs the FEWEST ROUNDS of the device's workgroup slots
 *                  (a 4K frame in 1024x8 tiles is 1080 workgroups on 1024 slots -- a second round that is 5 % full --
 *                  in 256x32 tiles 1020: 54.8 vs 47.9 % of peak frame by frame), the widest among equals.
 * Which class a launch over `nframes` frames falls into follows from the geometry alone.  mibayer_autotune[_list]
 * measures -- and the plan cache records -- the class of the launches it was given; mibayer_get_plan,
 * mibayer_plan_source and mibayer_ctx_variant_name describe the batch class; mibayer_set_plan / mibayer_copy_plan pin
 * every class.  The two below address the class of an `nframes`-frame launch; `source` receives MIBAYER_PLAN_*. */
int mibayer_get_plan_for (const mibayer_ctx *ctx, int nframes, int *variant, int *band, int *align_stores,
    int *source);
int mibayer_set_plan_for (mibayer_ctx *ctx, int nframes, int variant, int band, int align_stores);

/* Process-wide plan cache.  mibayer_autotune / mibayer_autotune_list record what
 * they measured under (device, width, height, src_stride, dst_stride, launch class);
 * mibayer_create of a stream with that geometry on that device (cfg.variant == 0)
 * starts from the recorded plan instead of the static default -- the second element
 * instance, the context after a renegotiation, the other three Bayer orders of one
 * camera do not measure again.  MIBAYER_PLAN_CACHE=0 in the environment turns
 * look-ups and recording off.  Reference analogue (set up once per process, reuse):
 * the once-guarded ORC programs, gst/bayer/gstbayerorc-dist.c:321-397. */
#define MIBAYER_PLAN_DEFAULT 0  /* the static per-geometry default of mibayer_create */
#define MIBAYER_PLAN_MEASURED 1 /* mibayer_autotune[_list] ran on this context       */
#define MIBAYER_PLAN_CACHED 2   /* taken from the process plan cache at create       */
#define MIBAYER_PLAN_SET 3      /* mibayer_set_plan / mibayer_copy_plan               */
int mibayer_plan_source (const mibayer_ctx *ctx);
/* Looks the context's geometry up in the cache again (a plan may have been measured
 * since the context was created): 1 = a cached plan was applied, 0 = none. */
int mibayer_plan_from_cache (mibayer_ctx *ctx);
void mibayer_plan_cache_clear (void);

/* ---- memory helpers --------------------------------------------------------- */

/* Pinned (hipHostMalloc) memory for buffer pools feeding the host path. */
void *mibayer_host_alloc (size_t bytes);
/* (while a context of this process is wedged -- a wait ran into its deadline and
 * the device has not caught up since -- the block goes on a deferred list instead
 * of hipHostFree, which would wait for that device; the list is returned to the
 * runtime as soon as no wedge is outstanding) */
void mibayer_host_free (void *p);
/* diagnostics: blocks on the deferred list / contexts whose device has not caught
 * up after a wait deadline (both poll, neither blocks) */
int mibayer_deferred_frees (void);
int mibayer_wedged_contexts (void);
/* The same, placed on the NUMA node next to HIP device `device` (the thread's
 * memory policy is set around a hipHostMallocNumaUser allocation): a pool that
 * feeds GPU k should not sit behind the socket link.  Falls back to
 * mibayer_host_alloc() when the node is unknown.  Free with mibayer_host_free(). */
void *mibayer_host_alloc_near (int device, size_t bytes);
/* 1 when p points into pinned / registered host memory (an asynchronous copy
 * from / to it really is asynchronous), 0 for ordinary pageable memory, where
 * hipMemcpyAsync blocks the caller while the runtime stages the data */
int mibayer_host_is_pinned (const void *p);
/* NUMA node next to a device (-1 = unknown) / holding the first page of p */
int mibayer_device_numa_node (int device);
int mibayer_host_numa_node (const void *p);

/* Device memory on the context's device, for C callers without another
 * allocator. */
void *mibayer_device_alloc (mibayer_ctx *ctx, size_t bytes);
void mibayer_device_free (mibayer_ctx *ctx, void *d_ptr);
int mibayer_copy_to_device (mibayer_ctx *ctx, void *d_dst, const void *src,
    size_t bytes);
int mibayer_copy_from_device (mibayer_ctx *ctx, void *dst, const void *d_src,
    size_t bytes);

/* Context-free device memory helpers (for a GstAllocator of device memory, the
 * `memory:HIPMemory` caps feature of gst/gstmihipmemory.c): synchronous. */
void *mibayer_dev_alloc (int device, size_t bytes);
void mibayer_dev_free (int device, void *d_ptr);
int mibayer_dev_upload (int device, void *d_dst, const void *src, size_t bytes);
int mibayer_dev_download (int device, void *dst, const void *d_src,
    size_t bytes);

/* Context-free copy queue and asynchronous upload, for an uploader that does
 * not want to wait for its DMA (gst/gstmihipelements.c, hipupload: the host
 * buffer is kept alive until the event recorded after the copy has fired, the
 * pattern of the reference tree's sys/nvcodec/gstcudaupload.c made
 * asynchronous).  `src` must stay valid until an event recorded on the stream
 * after the call has completed; from pageable memory the call itself blocks. */
void *mibayer_dev_stream_create (int device);
void mibayer_dev_stream_destroy (int device, void *hip_stream);
int mibayer_dev_upload_async (int device, void *d_dst, const void *src,
    size_t bytes, void *hip_stream);
/* the other direction (hipdownload's queued mode): `dst` is complete once an
 * event recorded on the stream after the call has fired */
int mibayer_dev_download_async (int device, void *dst, const void *d_src,
    size_t bytes, void *hip_stream);
/* 1 = the work recorded in the event has completed, 0 = not yet, < 0 = error */
int mibayer_dev_event_query (int device, void *event);

/* Context-free events, for stream-ordered hand-over of a device buffer from one
 * user to the next without a host round trip: record after the work that touches
 * the buffer, make the next user's stream wait for it -- or block the host on it.
 * (Plugin `mihip` records them lazily: one per stream when somebody has to wait
 * across queues or on the host, not one per buffer -- gst/gstmihipmemory.h.) */
void *mibayer_dev_event_create (int device);
void mibayer_dev_event_destroy (int device, void *event);
int mibayer_dev_event_record (int device, void *event,
    void *hip_stream /* used as given */);
int mibayer_dev_event_wait (int device, void *event);          /* host blocks */
int mibayer_dev_stream_wait_event (int device, void *hip_stream, void *event);

/* Counter-based synthetic mosaic generated on the device (stateless per byte;
 * definition in DESIGN.md "Synthetic input"): frames first_frame ..
 * first_frame+nframes-1 with the context's width/height/src_stride. */
int mibayer_fill_synthetic (mibayer_ctx *ctx, void *d_src,
    size_t src_frame_bytes, uint32_t first_frame, int nframes, uint32_t seed,
    void *hip_stream /* used as given, like mibayer_process_device */);

/* ---- introspection (tests) --------------------------------------------------- */

/* Number of kernel variants; variant ids are 0 .. n-1.  0 = "auto": the
 * production tile shape chosen from the stream width at mibayer_create(). */
int mibayer_variant_count (void);
const char *mibayer_variant_name (int variant);
/* the variant id "auto" (0) resolves to for a frame width by the padding rule (pure host arithmetic) */
int mibayer_auto_variant (int width);
/* ... for a launch of ONE frame of a sector-aligned geometry on a device with `compute_units` CUs: the production shape
 * whose grid needs the fewest rounds of the device's workgroup slots (4 per CU), the widest tile among equals (v5) */
int mibayer_frame_class_variant (int width, int height, int compute_units);
/* ... and the batch-class default of the common sensor widths whose measured winner the padding rule does not find:
 * 1 and (variant, band) if `width` is one of them, else 0 (v5) */
int mibayer_known_width_plan (int width, int *variant, int *band);
/* name of the concrete variant the context resolved to */
const char *mibayer_ctx_variant_name (const mibayer_ctx *ctx);
/* Pure host arithmetic, no device needed: the four v_perm_b32 selectors (output
 * pixel k = perm ({R'B' pair word, G word}, sel[k])) and the row-type swap that
 * mibayer_create() derives from (pattern, r_off, g_off, b_off) -- the kernel's
 * replacement for the reference's merge-function table and pointer swaps
 * (gstbayer2rgb.c:400-427).  Lets the byte-placement logic be checked on a CPU. */
int mibayer_plan_selectors (const mibayer_cfg *cfg, uint32_t sel[4],
    int *swap_rows);

/* Launch geometry the context would use for nframes frames: tile size in
 * pixels, tiles per tile row, tile rows in the batch (nframes * tiles_y), the
 * XCD band (tile rows per XCD band, 0 = identity map) and the grid size.  Any
 * pointer may be NULL. */
int mibayer_launch_geometry (const mibayer_ctx *ctx, int nframes, int *tile_w,
    int *tile_h, int *tiles_x, int64_t *tile_rows, int *band,
    int64_t *grid_blocks);
/* The XCD-aware block -> tile permutation used by the kernel, evaluated on the
 * host: linear tile id (tile_row * tiles_x + tx) that block `block` processes,
 * or -1 if that block idles. */
int64_t mibayer_block_to_tile (int64_t block, int tiles_x, int64_t tile_rows,
    int band);

#ifdef __cplusplus
}
#endif
#endif /* MIBAYER_H */
