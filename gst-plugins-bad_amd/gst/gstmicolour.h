/*
 * gstmicolour.h -- the colour-stage properties of bayer2rgb and hipbayer2rgb (MIBAYER_FLAG_COLOUR, include/mibayer.h):
 * black-level, red-/green-/blue-gain, ccm, tone-curve, gamma, and the automatic white balance on top of it:
 * white-balance (manual / grey-world) and awb-speed.  One definition for both plugins; each includes this header once,
 * after defining GST_MI_COLOUR_TONE_TYPE_NAME (the two plugins may be loaded into one process, so the enum types need
 * a name per plugin; the white-balance enum's is that name with "WhiteBalance" appended).
 *
 * With every property at its default an element does not set the flag: its output stays the reference's bytes.
 * white-balance=grey-world sets the flag on its own: the element measures every frame it gets back (1 x 1 mosaic zone
 * statistics, group `stats` of include/mibayer.h) and moves its red and blue gain towards the grey-world gains of that
 * frame (gst_mi_awb_step), for the frames it accepts afterwards.
 * exposure=auto sets the flag on its own too: the element reads the whole-frame mosaic histogram (group `hist`) of
 * every frame it gets back and moves a factor e on all three gains towards the one that puts the 99th percentile of
 * the brightest channel at ae-target (gst_mi_auto_step); ae-speed and ae-max-gain shape the loop.
 *
 * The colour entry points of libmibayer are bound WEAKLY: the plugins also load against builds of the library
 * interface that do not have them (the test doubles of tests/check), where a non-default colour request ends in an
 * element error and the defaults call none of them.
 */
#ifndef GST_MI_COLOUR_H
#define GST_MI_COLOUR_H

#include <gst/gst.h>
#include <stdlib.h>
#include <string.h>

#include "mibayer.h"

#pragma weak mibayer_colour_init
#pragma weak mibayer_colour_matrix
#pragma weak mibayer_colour_tone
#pragma weak mibayer_set_colour
#pragma weak mibayer_pool_set_colour
#pragma weak mibayer_stats_device
#pragma weak mibayer_set_stats
#pragma weak mibayer_frame_stats
#pragma weak mibayer_pool_set_stats
#pragma weak mibayer_pool_frame_stats
#pragma weak mibayer_stats_grey_world
#pragma weak mibayer_hist_device
#pragma weak mibayer_pool_set_hist
#pragma weak mibayer_pool_frame_hist
#pragma weak mibayer_hist_exposure

enum
{
  GST_MI_WHITE_BALANCE_MANUAL = 0,
  GST_MI_WHITE_BALANCE_GREY_WORLD
};

enum
{
  GST_MI_EXPOSURE_MANUAL = 0,
  GST_MI_EXPOSURE_AUTO
};

typedef struct
{
  guint black_level;
  gdouble gain[3];              /* red, green, blue */
  gchar *ccm;                   /* nine comma-separated numbers, row-major; NULL / "" = identity */
  gint tone_curve;              /* MIBAYER_TONE_* */
  gdouble gamma;
  gint white_balance;           /* GST_MI_WHITE_BALANCE_* */
  gdouble awb_speed;
  gint exposure;                /* GST_MI_EXPOSURE_* */
  gdouble ae_target, ae_speed, ae_max_gain;
} GstMiColourProps;

/* the running state of white-balance=grey-world: the red and blue gain in use (gst_mi_awb_start / gst_mi_awb_step) */
typedef struct
{
  gdouble gain[2];
} GstMiAwb;

/* the running state of exposure=auto: the factor on the three gains (1 to start with; gst_mi_auto_step) */
typedef struct
{
  gdouble e;
} GstMiAe;

/* the ids an element's property enum reserves, in this order, from its `first` id on */
enum
{
  GST_MI_COLOUR_PROP_BLACK_LEVEL = 0,
  GST_MI_COLOUR_PROP_RED_GAIN,
  GST_MI_COLOUR_PROP_GREEN_GAIN,
  GST_MI_COLOUR_PROP_BLUE_GAIN,
  GST_MI_COLOUR_PROP_CCM,
  GST_MI_COLOUR_PROP_TONE_CURVE,
  GST_MI_COLOUR_PROP_GAMMA,
  GST_MI_COLOUR_PROP_WHITE_BALANCE,
  GST_MI_COLOUR_PROP_AWB_SPEED,
  GST_MI_COLOUR_PROP_EXPOSURE,
  GST_MI_COLOUR_PROP_AE_TARGET,
  GST_MI_COLOUR_PROP_AE_SPEED,
  GST_MI_COLOUR_PROP_AE_MAX_GAIN,
  GST_MI_COLOUR_N_PROPS
};

#define GST_MI_COLOUR_DEFAULT_GAMMA 2.2
#define GST_MI_COLOUR_DEFAULT_AWB_SPEED 0.25
#define GST_MI_COLOUR_DEFAULT_AE_TARGET 0.9
#define GST_MI_COLOUR_DEFAULT_AE_SPEED 0.25
#define GST_MI_COLOUR_DEFAULT_AE_MAX_GAIN 4.0
#define GST_MI_AE_FRACTION 0.99

static GType
gst_mi_colour_exposure_get_type (void)
{
  static gsize type = 0;
  static const GEnumValue values[] = {
    {GST_MI_EXPOSURE_MANUAL, "Manual: the gain properties as they are", "manual"},
    {GST_MI_EXPOSURE_AUTO, "Auto: one factor on all gains follows the histogram of the frames", "auto"},
    {0, NULL, NULL}
  };
  if (g_once_init_enter (&type)) {
    GType t = g_enum_register_static (GST_MI_COLOUR_TONE_TYPE_NAME "Exposure", values);
    g_once_init_leave (&type, t);
  }
  return (GType) type;
}

static GType
gst_mi_colour_white_balance_get_type (void)
{
  static gsize type = 0;
  static const GEnumValue values[] = {
    {GST_MI_WHITE_BALANCE_MANUAL, "Manual: the red-/green-/blue-gain properties", "manual"},
    {GST_MI_WHITE_BALANCE_GREY_WORLD,
        "Grey world: red and blue gain follow the channel means of the frames", "grey-world"},
    {0, NULL, NULL}
  };
  if (g_once_init_enter (&type)) {
    GType t = g_enum_register_static (GST_MI_COLOUR_TONE_TYPE_NAME "WhiteBalance", values);
    g_once_init_leave (&type, t);
  }
  return (GType) type;
}

static GType
gst_mi_colour_tone_get_type (void)
{
  static gsize type = 0;
  static const GEnumValue values[] = {
    {MIBAYER_TONE_LINEAR, "Linear: no tone curve", "linear"},
    {MIBAYER_TONE_SRGB, "The sRGB transfer function", "srgb"},
    {MIBAYER_TONE_GAMMA, "Power law x^(1/gamma), see the gamma property", "gamma"},
    {0, NULL, NULL}
  };
  if (g_once_init_enter (&type)) {
    GType t = g_enum_register_static (GST_MI_COLOUR_TONE_TYPE_NAME, values);
    g_once_init_leave (&type, t);
  }
  return (GType) type;
}

static void
gst_mi_colour_props_init (GstMiColourProps * p)
{
  p->black_level = 0;
  p->gain[0] = p->gain[1] = p->gain[2] = 1.0;
  p->ccm = NULL;
  p->tone_curve = MIBAYER_TONE_LINEAR;
  p->gamma = GST_MI_COLOUR_DEFAULT_GAMMA;
  p->white_balance = GST_MI_WHITE_BALANCE_MANUAL;
  p->awb_speed = GST_MI_COLOUR_DEFAULT_AWB_SPEED;
  p->exposure = GST_MI_EXPOSURE_MANUAL;
  p->ae_target = GST_MI_COLOUR_DEFAULT_AE_TARGET;
  p->ae_speed = GST_MI_COLOUR_DEFAULT_AE_SPEED;
  p->ae_max_gain = GST_MI_COLOUR_DEFAULT_AE_MAX_GAIN;
}

static void
gst_mi_colour_props_clear (GstMiColourProps * p)
{
  g_free (p->ccm);
  p->ccm = NULL;
}

/* dst = src (dst holds a valid or NULL ccm) */
static G_GNUC_UNUSED void
gst_mi_colour_props_copy (GstMiColourProps * dst, const GstMiColourProps * src)
{
  gchar *ccm = g_strdup (src->ccm);
  g_free (dst->ccm);
  *dst = *src;
  dst->ccm = ccm;
}

/* gamma alone changes nothing: it is read by tone-curve=gamma only (and awb-speed by white-balance=grey-world, the
 * ae-* properties by exposure=auto) */
static gboolean
gst_mi_colour_props_are_default (const GstMiColourProps * p)
{
  return p->black_level == 0 && p->gain[0] == 1.0 && p->gain[1] == 1.0 && p->gain[2] == 1.0
      && (p->ccm == NULL || p->ccm[0] == '\0') && p->tone_curve == MIBAYER_TONE_LINEAR
      && p->white_balance == GST_MI_WHITE_BALANCE_MANUAL && p->exposure == GST_MI_EXPOSURE_MANUAL;
}

/* The mibayer_colour of the properties, built with the library's helpers so that everybody rounds alike.  FALSE with a
 * message (g_free) when the ccm string does not parse, a value is out of range or the library has no colour stage. */
static gboolean
gst_mi_colour_props_build (const GstMiColourProps * p, mibayer_colour * out, gchar ** message)
{
  double ccm[9];
  gboolean have_ccm = p->ccm != NULL && p->ccm[0] != '\0';

  *message = NULL;
  if (!mibayer_colour_init || !mibayer_colour_matrix || !mibayer_colour_tone) {
    *message = g_strdup ("this libmibayer has no colour stage (mibayer_colour_* are missing)");
    return FALSE;
  }
  if (have_ccm) {
    const gchar *s = p->ccm;
    gint k;
    for (k = 0; k < 9; k++) {
      gchar *end = NULL;
      ccm[k] = g_ascii_strtod (s, &end);
      if (end == s)
        break;
      s = end;
      while (*s == ' ')
        s++;
      if (k < 8) {
        if (*s != ',')
          break;
        s++;
      }
    }
    if (k < 9 || *s != '\0') {
      *message = g_strdup_printf ("ccm=\"%s\" is not nine comma-separated numbers", p->ccm);
      return FALSE;
    }
  }
  mibayer_colour_init (out);
  out->black[0] = out->black[1] = out->black[2] = (int32_t) p->black_level;
  if (mibayer_colour_matrix (p->gain, have_ccm ? ccm : NULL, out->matrix) != MIBAYER_OK) {
    *message = g_strdup ("gains x ccm leave the matrix range (-15.99 .. 15.99 per entry)");
    return FALSE;
  }
  if (p->tone_curve != MIBAYER_TONE_LINEAR) {
    if (mibayer_colour_tone (p->tone_curve, p->gamma, out->tone) != MIBAYER_OK) {
      *message = g_strdup_printf ("tone-curve %d with gamma=%g is not valid", p->tone_curve, p->gamma);
      return FALSE;
    }
    out->has_tone = 1;
  }
  return TRUE;
}

/* white-balance=grey-world: the sample range of the 1 x 1 statistics at `depth` bits, and the gains to start from */
static G_GNUC_UNUSED void
gst_mi_awb_start (const GstMiColourProps * p, GstMiAwb * awb, gint depth, guint32 * lo, guint32 * hi)
{
  const guint32 vmax = (1u << depth) - 1u;

  awb->gain[0] = p->gain[0];
  awb->gain[1] = p->gain[2];
  *lo = MAX (p->black_level, 1u);
  *hi = vmax - (vmax >> 4);
}

/* One step of the loop on the 1 x 1 statistics of a frame: the targets are green-gain x the grey-world gains of the
 * frame, and each gain moves by awb-speed x (target - gain).  TRUE with the stage to use from now on in `out`; FALSE
 * when nothing changes (the helper found no usable mean, or the new matrix would leave its range). */
static G_GNUC_UNUSED gboolean
gst_mi_awb_step (const GstMiColourProps * p, GstMiAwb * awb, const mibayer_stats_zone * zone, gint pattern,
    mibayer_colour * out)
{
  const double black[3] = { p->black_level, p->black_level, p->black_level };
  double gw[3];
  GstMiColourProps q = *p;      /* shares the ccm string: not cleared */
  gchar *why = NULL;
  gint k;

  if (!mibayer_stats_grey_world || mibayer_stats_grey_world (zone, 1, pattern, black, gw) != 1)
    return FALSE;
  for (k = 0; k < 2; k++) {
    const gdouble g = awb->gain[k] + p->awb_speed * (p->gain[1] * gw[2 * k] - awb->gain[k]);
    q.gain[2 * k] = CLAMP (g, 0.0, 15.99);
  }
  if (!gst_mi_colour_props_build (&q, out, &why)) {
    g_free (why);
    return FALSE;
  }
  awb->gain[0] = q.gain[0];
  awb->gain[1] = q.gain[2];
  return TRUE;
}

/* One step of the loops of an element with exposure=auto, on what it measured of a frame: `zone` (NULL unless
 * white-balance=grey-world is on as well: that step runs first, as in gst_mi_awb_step, and its gains are the current
 * ones) and the whole-frame histogram `hist`.  x = mibayer_hist_exposure (hist, black-level, the current gains before
 * e, 0.99, ae-target, ae-max-gain); e += ae-speed x (x - e); the stage gets gain_k x e, clamped to the gain range.  TRUE
 * with the stage to use from now on in `out`; FALSE when nothing changes (neither helper had an answer, or the new matrix
 * would leave its range). */
static G_GNUC_UNUSED gboolean
gst_mi_auto_step (const GstMiColourProps * p, GstMiAwb * awb, GstMiAe * ae, const mibayer_stats_zone * zone,
    const mibayer_hist * hist, gint pattern, gint depth, mibayer_colour * out)
{
  const double black[3] = { p->black_level, p->black_level, p->black_level };
  double gw[3], x, e = ae->e;
  GstMiColourProps q = *p, r;   /* share the ccm string: not cleared */
  gboolean moved = FALSE;
  gchar *why = NULL;
  gint k;

  if (p->white_balance == GST_MI_WHITE_BALANCE_GREY_WORLD) {
    q.gain[0] = awb->gain[0];
    q.gain[2] = awb->gain[1];
    if (zone && mibayer_stats_grey_world && mibayer_stats_grey_world (zone, 1, pattern, black, gw) == 1) {
      for (k = 0; k < 2; k++) {
        const gdouble g = awb->gain[k] + p->awb_speed * (p->gain[1] * gw[2 * k] - awb->gain[k]);
        q.gain[2 * k] = CLAMP (g, 0.0, 15.99);
      }
      moved = TRUE;
    }
  }
  if (hist && mibayer_hist_exposure && mibayer_hist_exposure (hist, pattern, depth, black, q.gain, GST_MI_AE_FRACTION,
          p->ae_target, p->ae_max_gain, &x) == 1) {
    e += p->ae_speed * (x - e);
    moved = TRUE;
  }
  if (!moved)
    return FALSE;
  r = q;
  for (k = 0; k < 3; k++) {
    const gdouble g = q.gain[k] * e;
    r.gain[k] = CLAMP (g, 0.0, 15.99);
  }
  if (!gst_mi_colour_props_build (&r, out, &why)) {
    g_free (why);
    return FALSE;
  }
  awb->gain[0] = q.gain[0];
  awb->gain[1] = q.gain[2];
  ae->e = e;
  return TRUE;
}

static void
gst_mi_colour_install_properties (GObjectClass * object_class, guint first)
{
  const GParamFlags flags = G_PARAM_READWRITE | GST_PARAM_MUTABLE_READY | G_PARAM_STATIC_STRINGS;
  static const gchar *const gain_name[3] = { "red-gain", "green-gain", "blue-gain" };
  static const gchar *const gain_nick[3] = { "Red gain", "Green gain", "Blue gain" };
  gint k;

  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_BLACK_LEVEL,
      g_param_spec_uint ("black-level", "Black level",
          "Subtracted from every demosaiced channel, at the sensor's native depth "
          "(colour stage fused into the demosaic kernel; any non-default colour "
          "property turns it on, and the output is then no longer the stock element's)",
          0, 65535, 0, flags));
  for (k = 0; k < 3; k++)
    g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_RED_GAIN + k,
        g_param_spec_double (gain_name[k], gain_nick[k],
            "White-balance gain of the channel, applied before ccm", 0.0, 15.99, 1.0, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_CCM,
      g_param_spec_string ("ccm", "Colour correction matrix",
          "Nine comma-separated numbers, row-major (output R, G, B from input R, G, B); "
          "empty = identity.  gains x ccm entries must stay within +-15.99", "", flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_TONE_CURVE,
      g_param_spec_enum ("tone-curve", "Tone curve",
          "Transfer curve applied after the matrix", gst_mi_colour_tone_get_type (),
          MIBAYER_TONE_LINEAR, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_GAMMA,
      g_param_spec_double ("gamma", "Gamma",
          "Exponent of tone-curve=gamma: out = in^(1/gamma)", 0.01, 100.0,
          GST_MI_COLOUR_DEFAULT_GAMMA, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_WHITE_BALANCE,
      g_param_spec_enum ("white-balance", "White balance",
          "manual: the gain properties as they are; grey-world: turns the colour stage on, measures "
          "every frame and moves red-gain / blue-gain (the starting values) towards green-gain x the "
          "grey-world gains of the frame, for the frames accepted afterwards",
          gst_mi_colour_white_balance_get_type (), GST_MI_WHITE_BALANCE_MANUAL, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_AWB_SPEED,
      g_param_spec_double ("awb-speed", "AWB speed",
          "white-balance=grey-world: gain += awb-speed x (target - gain) after every frame; 1 = jump",
          G_MINDOUBLE, 1.0, GST_MI_COLOUR_DEFAULT_AWB_SPEED, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_EXPOSURE,
      g_param_spec_enum ("exposure", "Exposure",
          "manual: the gain properties as they are; auto: turns the colour stage on, reads the mosaic "
          "histogram of every frame and moves one factor on all three gains so that the 99th percentile "
          "of the brightest channel lands on ae-target, for the frames accepted afterwards",
          gst_mi_colour_exposure_get_type (), GST_MI_EXPOSURE_MANUAL, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_AE_TARGET,
      g_param_spec_double ("ae-target", "AE target",
          "exposure=auto: where the 99th percentile should sit, as a fraction of full scale",
          G_MINDOUBLE, 1.0, GST_MI_COLOUR_DEFAULT_AE_TARGET, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_AE_SPEED,
      g_param_spec_double ("ae-speed", "AE speed",
          "exposure=auto: factor += ae-speed x (wanted - factor) after every frame; 1 = jump",
          G_MINDOUBLE, 1.0, GST_MI_COLOUR_DEFAULT_AE_SPEED, flags));
  g_object_class_install_property (object_class, first + GST_MI_COLOUR_PROP_AE_MAX_GAIN,
      g_param_spec_double ("ae-max-gain", "AE maximum gain",
          "exposure=auto: the largest factor the loop asks for", 1.0, 15.99,
          GST_MI_COLOUR_DEFAULT_AE_MAX_GAIN, flags));
}

/* TRUE when `id` (relative to the element's first colour id) is a colour property; the caller holds its lock */
static gboolean
gst_mi_colour_set_property (GstMiColourProps * p, gint id, const GValue * value)
{
  switch (id) {
    case GST_MI_COLOUR_PROP_BLACK_LEVEL:
      p->black_level = g_value_get_uint (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_RED_GAIN:
    case GST_MI_COLOUR_PROP_GREEN_GAIN:
    case GST_MI_COLOUR_PROP_BLUE_GAIN:
      p->gain[id - GST_MI_COLOUR_PROP_RED_GAIN] = g_value_get_double (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_CCM:
      g_free (p->ccm);
      p->ccm = g_value_dup_string (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_TONE_CURVE:
      p->tone_curve = g_value_get_enum (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_GAMMA:
      p->gamma = g_value_get_double (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_WHITE_BALANCE:
      p->white_balance = g_value_get_enum (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_AWB_SPEED:
      p->awb_speed = g_value_get_double (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_EXPOSURE:
      p->exposure = g_value_get_enum (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_AE_TARGET:
      p->ae_target = g_value_get_double (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_AE_SPEED:
      p->ae_speed = g_value_get_double (value);
      return TRUE;
    case GST_MI_COLOUR_PROP_AE_MAX_GAIN:
      p->ae_max_gain = g_value_get_double (value);
      return TRUE;
    default:
      return FALSE;
  }
}

static gboolean
gst_mi_colour_get_property (const GstMiColourProps * p, gint id, GValue * value)
{
  switch (id) {
    case GST_MI_COLOUR_PROP_BLACK_LEVEL:
      g_value_set_uint (value, p->black_level);
      return TRUE;
    case GST_MI_COLOUR_PROP_RED_GAIN:
    case GST_MI_COLOUR_PROP_GREEN_GAIN:
    case GST_MI_COLOUR_PROP_BLUE_GAIN:
      g_value_set_double (value, p->gain[id - GST_MI_COLOUR_PROP_RED_GAIN]);
      return TRUE;
    case GST_MI_COLOUR_PROP_CCM:
      g_value_set_string (value, p->ccm ? p->ccm : "");
      return TRUE;
    case GST_MI_COLOUR_PROP_TONE_CURVE:
      g_value_set_enum (value, p->tone_curve);
      return TRUE;
    case GST_MI_COLOUR_PROP_GAMMA:
      g_value_set_double (value, p->gamma);
      return TRUE;
    case GST_MI_COLOUR_PROP_WHITE_BALANCE:
      g_value_set_enum (value, p->white_balance);
      return TRUE;
    case GST_MI_COLOUR_PROP_AWB_SPEED:
      g_value_set_double (value, p->awb_speed);
      return TRUE;
    case GST_MI_COLOUR_PROP_EXPOSURE:
      g_value_set_enum (value, p->exposure);
      return TRUE;
    case GST_MI_COLOUR_PROP_AE_TARGET:
      g_value_set_double (value, p->ae_target);
      return TRUE;
    case GST_MI_COLOUR_PROP_AE_SPEED:
      g_value_set_double (value, p->ae_speed);
      return TRUE;
    case GST_MI_COLOUR_PROP_AE_MAX_GAIN:
      g_value_set_double (value, p->ae_max_gain);
      return TRUE;
    default:
      return FALSE;
  }
}

#endif /* GST_MI_COLOUR_H */
