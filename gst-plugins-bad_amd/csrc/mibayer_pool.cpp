/*
 * mibayer_pool -- round-robin frame sharding over GPUs (include/mibayer.h,
 * "multi-GPU frame sharding").  Pure host logic: no HIP call in this file, the
 * devices are reached through the per-context ABI and csrc/mibayer_hooks.h
 * only, so the same code runs over a test double of the contexts under
 * AddressSanitizer / ThreadSanitizer (tests/test_pool_logic.py).
 *
 * Frames are independent (the reference keeps no state between frames,
 * gstbayer2rgb.c:387-451): frame g goes to the next device in rotation and the
 * results come back in submission order.  On top of that, three things a
 * production multi-GPU stream needs:
 *
 *  - FAILOVER.  The reference's only failure handling on this path is "warn and
 *    carry on" (gstbayer2rgb.c:484-486).  Here a device whose context reports
 *    MIBAYER_ERR_HIP / MIBAYER_ERR_NOMEM is dropped from the rotation, the
 *    frames it still held are converted again on the surviving devices (same
 *    bytes: the conversion is a pure function of the frame), order is kept, and
 *    the event is reported once (mibayer_pool_take_failure).  The stream fails
 *    only when no device is left.
 *
 *  - PAGEABLE BUFFERS.  hipMemcpyAsync from / to pageable memory blocks the
 *    calling thread while the runtime stages it, so one streaming thread would
 *    feed N GPUs one after the other.  In a pool of more than one shard, the
 *    first frame whose source or destination is pageable turns its shard over to
 *    a helper thread (one per shard, started on first use): from then on the
 *    helper drives that context's submit / wait ring -- so uploads, kernels and
 *    downloads of consecutive frames keep overlapping inside the shard -- and
 *    the streaming thread only queues and, at wait time, blocks on the oldest
 *    frame.  Shards that only ever see pinned frames keep the direct,
 *    enqueue-only path, and so does a single-shard pool (a helper would add a
 *    hand-off and no parallelism).  (A second CPU copy through a pinned bounce
 *    buffer was rejected: the runtime's own staging moves ~40 GB/s, a memcpy
 *    thread ~10.)
 *
 *  - DEADLINES.  A device that stops answering completes nothing: every wait of a context is bounded
 *    (mibayer_set_wait_timeout), MIBAYER_ERR_TIMEOUT counts as a device failure like MIBAYER_ERR_HIP, and a
 *    context that timed out is never waited for again (mibayer_internal_abandon returns at once for it).
 *
 *  - NUMA-LOCAL ROUTING.  On a two-socket node a frame whose pinned buffer sits next to GPU k should go to GPU k:
 *    when the shards' devices span more than one NUMA node, a frame is routed to the live shard on the node that
 *    holds its 4-byte-per-pixel buffer as long as that keeps the rotation balanced (no shard more than its in-flight
 *    share ahead); otherwise, and whenever the node is unknown, strictly g mod N.  Results keep submission order.
 *
 *  - A SUBMIT THREAD PER SHARD (MIBAYER_POOL_THREADS=1): every shard is driven by its helper thread from the start,
 *    pinned frames included, so N GPUs are fed by N host threads instead of the one streaming thread.
 *
 *  - FAULT INJECTION for drills and tests: mibayer_pool_inject_fault() /
 *    MIBAYER_INJECT_FAULT=shard:frames make a shard report a device error after
 *    it has completed that many frames; mibayer_pool_inject_stall() /
 *    MIBAYER_INJECT_STALL=shard:frames:ms occupy a shard's compute queue for `ms`
 *    milliseconds once `frames` frames have been routed to it.
 */
#include "mibayer_hooks.h"

/* the context layer's colour entry points are bound weakly: the pool logic also links against test doubles of that
 * layer that do not have them (tests/check), where a colour request is refused */
#pragma weak mibayer_set_colour
#pragma weak mibayer_get_colour
/* ... and so are the statistics': a pool over such a double refuses mibayer_pool_set_stats */
#pragma weak mibayer_set_stats
#pragma weak mibayer_frame_stats
/* ... and the histogram's: mibayer_pool_set_hist is refused there too */
#pragma weak mibayer_set_hist
#pragma weak mibayer_frame_hist
/* ... and the focus statistics': mibayer_pool_set_focus is refused there too */
#pragma weak mibayer_set_focus
#pragma weak mibayer_frame_focus
/* ... and the shading table's: mibayer_pool_set_shading is refused there too */
#pragma weak mibayer_set_shading
/* ... and the defective pixel correction's: mibayer_pool_set_dpc is refused there too */
#pragma weak mibayer_set_dpc
/* ... and the noise reduction's: mibayer_pool_set_nr is refused there too */
#pragma weak mibayer_set_nr

#include <sched.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

/* what mibayer_pool_set_stats, mibayer_pool_set_hist and mibayer_pool_set_focus asked for, together: one record per
 * frame carries all three */
struct StatsGrid {
  int zones_x, zones_y;         /* (0, 0): no zones */
  uint32_t lo, hi;
  int hist, x0, y0, w, h;       /* hist = 0: no histogram */
  int fzones_x, fzones_y;       /* (0, 0): no focus zones */
  uint32_t thr;
};
/* what mibayer_pool_set_shading asked for: the parameters and the pool's copy of the table (par.table points into it) */
struct ShadeSet {
  mibayer_shading par;
  std::vector<uint16_t> table;
};
/* what mibayer_pool_set_dpc asked for: the parameters and the pool's copy of the list (par.defects points into it) */
struct DpcAsk {
  mibayer_dpc par;
  std::vector<uint32_t> list;
};
/* a frame's histogram rides behind its zones in the same vector, as it does in a context's slot */
constexpr size_t kHistZones = sizeof (mibayer_hist) / sizeof (mibayer_stats_zone);
/* ... and its focus zones behind the histogram, in as many elements of the vector as hold them */
inline size_t focus_span (size_t nf)
{
  return (nf * sizeof (mibayer_focus_zone) + sizeof (mibayer_stats_zone) - 1) / sizeof (mibayer_stats_zone);
}

enum FrameState {
  F_DIRECT,     /* in the ring of its shard's context, submitted by the streaming thread */
  F_QUEUED,     /* in the job queue of its shard's helper thread                  */
  F_RUNNING,    /* the helper thread has it (being submitted, or in the context's ring) */
  F_DONE,       /* converted by a helper thread (or by a synchronous re-do)       */
  F_FAILED,     /* the helper thread got a device error for it                    */
  F_REDO,       /* its device failed: convert again on a surviving device         */
  F_LOST        /* it was in flight on a device that ran into the wait deadline: the
                   device may still read / write its buffers, so it is neither converted
                   again into them nor handed back as done (mibayer_pool_reclaim)      */
};

struct Frame {
  const uint8_t *src;
  uint8_t *dst;
  void *tag;
  int shard;    /* where it is (being) converted  */
  int owner;    /* whose in-flight budget it uses */
  int state;    /* FrameState; helper-thread frames: under Shard::mu */
  int rc;
  bool submitted;       /* handed to the context of `shard` (its ring may hold it) */
  /* MIBAYER_FLAG_COLOUR pools: the stage the pool held when mibayer_pool_submit accepted the frame; whoever hands the
   * frame to a context -- the caller's thread, a helper thread later, a redo on another shard -- applies it first */
  std::shared_ptr<const mibayer_colour> colour;
  /* mibayer_pool_set_stats: the grid the pool held when the frame was accepted (NULL: none), applied like the stage;
   * and the frame's zones, fetched from the context by the thread that retired the frame there */
  std::shared_ptr<const StatsGrid> grid;
  std::vector<mibayer_stats_zone> zones;
  /* mibayer_pool_set_shading: the table the pool held when the frame was accepted (NULL: none), applied like the stage */
  std::shared_ptr<const ShadeSet> shade;
  std::shared_ptr<const DpcAsk> dpc;            /* mibayer_pool_set_dpc: likewise */
  std::shared_ptr<const mibayer_nr> nr;         /* mibayer_pool_set_nr: likewise */
};

struct Shard {
  mibayer_ctx *ctx = nullptr;
  int device = 0;
  bool alive = true;
  int inflight = 0;             /* frames owned and not yet handed back (streaming thread) */
  int node = -1;                /* NUMA node next to the device; -1 unknown */
  long long assigned = 0;       /* frames routed here so far (balance of the NUMA-local routing) */
  long long stall_after = -1;   /* MIBAYER_INJECT_STALL: stall the compute queue once this many frames were routed here */
  int stall_ms = 0;
  std::shared_ptr<const mibayer_colour> applied;        /* the stage its context holds (touched by whichever ONE
                                                           thread hands frames to the context) */
  std::shared_ptr<const StatsGrid> applied_grid;        /* ... and the statistics grid (NULL: off, as created) */
  std::shared_ptr<const ShadeSet> applied_shade;        /* ... and the shading table (NULL: off, as created) */
  std::shared_ptr<const DpcAsk> applied_dpc;            /* ... and the defective pixel correction (likewise) */
  std::shared_ptr<const mibayer_nr> applied_nr;         /* ... and the noise reduction curve (likewise) */
  std::atomic<long long> completions { 0 };
  std::atomic<long long> fail_after { -1 };     /* fault injection; -1 = never */
  /* helper thread */
  std::thread th;
  bool th_started = false;
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  std::deque<Frame *> jobs;     /* waiting for room in the context's ring             */
  std::deque<Frame *> ring;     /* in the context's ring, oldest first (helper mode)  */
  bool helper_mode = false;     /* the helper thread owns the context's submit / wait */
  bool pageable_seen = false;   /* a pageable frame came by: the context has queues of its own */
  int ring_room = 2;            /* stream.inflight                                     */
  bool quit = false;
  bool broken = false;
  bool timed_out = false;       /* what broke it was a wait deadline */
  int helper_lost = 0;          /* frames its helper thread marked F_LOST (for the failure note) */
  char errmsg[200] = "";

  /* true exactly once, when the shard has completed `fail_after` frames */
  bool fault_due ()
  {
    const long long n = ++completions;
    const long long at = fail_after.load ();
    return at >= 0 && n > at;
  }
};

/* the context of `sh` gets the frame's colour stage unless it holds it already: call right before the frame is handed
 * to the context, on the thread that hands it over */
void apply_colour (Shard *sh, const Frame *f)
{
  if (!f->colour || f->colour == sh->applied || !mibayer_set_colour)
    return;
  if (mibayer_set_colour (sh->ctx, f->colour.get ()) == MIBAYER_OK)
    sh->applied = f->colour;
}

/* the same for the frame's shading table: a frame converted again on another shard is shaded there with its own.
 * mibayer_pool_set_shading has checked the table by the context's own rules, so what can fail here is the device
 * (allocation, upload).  As with the stage, the frame is then converted with what the context holds, and the table is
 * tried again with the next frame; a device that is really gone fails the frame's submit and is dropped there. */
void apply_shading (Shard *sh, const Frame *f)
{
  if (f->shade == sh->applied_shade || !mibayer_set_shading)
    return;
  if (mibayer_set_shading (sh->ctx, f->shade ? &f->shade->par : NULL) == MIBAYER_OK)
    sh->applied_shade = f->shade;
}

/* the same for the frame's defective pixel correction */
void apply_dpc (Shard *sh, const Frame *f)
{
  if (f->dpc == sh->applied_dpc || !mibayer_set_dpc)
    return;
  if (mibayer_set_dpc (sh->ctx, f->dpc ? &f->dpc->par : NULL) == MIBAYER_OK)
    sh->applied_dpc = f->dpc;
}

/* the same for the frame's noise reduction curve */
void apply_nr (Shard *sh, const Frame *f)
{
  if (f->nr == sh->applied_nr || !mibayer_set_nr)
    return;
  if (mibayer_set_nr (sh->ctx, f->nr.get ()) == MIBAYER_OK)
    sh->applied_nr = f->nr;
}

/* the same for the frame's statistics grid (and, with it, the shading table: the two travel together) */
void apply_stats (Shard *sh, const Frame *f)
{
  apply_shading (sh, f);
  apply_dpc (sh, f);
  apply_nr (sh, f);
  if (f->grid == sh->applied_grid || !mibayer_set_stats)
    return;
  const StatsGrid off = {};
  const StatsGrid *g = f->grid ? f->grid.get () : &off;
  bool ok = mibayer_set_stats (sh->ctx, g->zones_x, g->zones_y, g->lo, g->hi) == MIBAYER_OK;
  if (mibayer_set_hist)
    ok = mibayer_set_hist (sh->ctx, g->hist, g->x0, g->y0, g->w, g->h) == MIBAYER_OK && ok;
  if (mibayer_set_focus)
    ok = mibayer_set_focus (sh->ctx, g->fzones_x, g->fzones_y, g->thr) == MIBAYER_OK && ok;
  if (ok)
    sh->applied_grid = f->grid;
}

/* the zones, then the histogram, then the focus zones of the frame the context of `sh` handed back last; empty when it has neither */
void read_stats (Shard *sh, const StatsGrid *g, std::vector<mibayer_stats_zone> *z)
{
  z->clear ();
  if (!g || !mibayer_frame_stats)
    return;
  const size_t nz = (size_t) g->zones_x * (size_t) g->zones_y;
  const size_t nh = g->hist ? kHistZones : 0, nf = (size_t) g->fzones_x * (size_t) g->fzones_y;
  z->resize (nz + nh + focus_span (nf));
  bool ok = nz == 0 || mibayer_frame_stats (sh->ctx, z->data (), (int) nz) == MIBAYER_OK;
  if (g->hist)
    ok = ok && mibayer_frame_hist && mibayer_frame_hist (sh->ctx, (mibayer_hist *) (z->data () + nz)) == MIBAYER_OK;
  if (nf)
    ok = ok && mibayer_frame_focus
        && mibayer_frame_focus (sh->ctx, (mibayer_focus_zone *) (z->data () + nz + nh), (int) nf) == MIBAYER_OK;
  if (!ok)
    z->clear ();
}

/* the context of `sh` has just handed the frame back to this thread: keep its zones with the frame */
void fetch_stats (Shard *sh, Frame *f)
{
  read_stats (sh, f->grid.get (), &f->zones);
}

bool device_failure (int rc)
{
  return rc == MIBAYER_ERR_HIP || rc == MIBAYER_ERR_NOMEM || rc == MIBAYER_ERR_TIMEOUT;
}

/* everything the helper still holds is re-done elsewhere (mu held) -- except, after a wait deadline, the frames
 * the context already has: those are lost (F_LOST).  kill_shard() has the last word on which of the two it is. */
void helper_give_up (Shard *sh, const char *why, bool timed_out = false)
{
  sh->broken = true;
  sh->timed_out = sh->timed_out || timed_out;
  if (why != sh->errmsg)
    snprintf (sh->errmsg, sizeof sh->errmsg, "%s", why ? why : "");
  for (Frame *f : sh->ring) {
    f->state = (sh->timed_out && f->submitted) ? F_LOST : F_REDO;
    sh->helper_lost += f->state == F_LOST ? 1 : 0;
  }
  sh->ring.clear ();
  for (Frame *f : sh->jobs)
    f->state = F_REDO;
  sh->jobs.clear ();
  sh->cv_done.notify_all ();
}

/* Helper mode: this thread is the only caller of the context's submit / wait.
 * It keeps the ring as full as the queue allows (a submit from pageable memory
 * blocks while the runtime stages the upload -- that is the point of being on a
 * thread of its own) and retires the oldest frame whenever nothing can be
 * submitted. */
/* A shard's thread runs on the CPUs of the NUMA node next to its GPU (hard part 7: "per-GPU
 * threads, NUMA-local pinned buffers"): its staging copies and the runtime's submission path then touch memory of
 * that socket only.  Best effort -- the node's CPU list comes from sysfs; nothing happens when the node is unknown,
 * the list cannot be read, or none of its CPUs is in the thread's current mask.  MIBAYER_POOL_PIN_THREADS=0: off. */
void pin_to_node (int node)
{
  if (node < 0)
    return;
  if (const char *e = getenv ("MIBAYER_POOL_PIN_THREADS"))
    if (atoi (e) == 0)
      return;
  char path[96];
  snprintf (path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen (path, "r");
  if (!f)
    return;
  char list[4096];
  const size_t n = fread (list, 1, sizeof list - 1, f);
  fclose (f);
  list[n] = 0;
  cpu_set_t allowed, want;
  CPU_ZERO (&want);
  if (sched_getaffinity (0, sizeof allowed, &allowed) != 0)
    return;
  int count = 0;
  for (char *q = list; *q;) {           /* "0-63,128-191" */
    char *end = NULL;
    const long a = strtol (q, &end, 10);
    if (end == q)
      break;
    long b = a;
    if (*end == '-') {
      q = end + 1;
      b = strtol (q, &end, 10);
      if (end == q)
        break;
    }
    for (long c = a; c <= b && c < CPU_SETSIZE; c++)
      if (c >= 0 && CPU_ISSET ((int) c, &allowed)) {
        CPU_SET ((int) c, &want);
        count++;
      }
    q = (*end == ',') ? end + 1 : end;
    if (*end != ',' )
      break;
  }
  if (count > 0)
    (void) sched_setaffinity (0, sizeof want, &want);
}

void helper_main (Shard *sh)
{
  pin_to_node (sh->node);
  std::unique_lock<std::mutex> lk (sh->mu);
  for (;;) {
    sh->cv_job.wait (lk, [sh] {
      return sh->quit || !sh->jobs.empty () || !sh->ring.empty ();
    });
    if (sh->quit && sh->jobs.empty () && sh->ring.empty ())
      return;
    if (sh->broken) {
      helper_give_up (sh, sh->errmsg);
      continue;
    }
    if (!sh->jobs.empty () && (int) sh->ring.size () < sh->ring_room) {
      Frame *f = sh->jobs.front ();
      sh->jobs.pop_front ();
      f->state = F_RUNNING;
      f->submitted = true;      /* from here on the context may hold it */
      sh->ring.push_back (f);
      lk.unlock ();
      apply_colour (sh, f);
      apply_stats (sh, f);
      const int rc = mibayer_submit (sh->ctx, f->src, f->dst, f);
      lk.lock ();
      if (rc != MIBAYER_OK) {
        f->rc = rc;
        f->submitted = false;   /* a failed submit leaves nothing of the frame behind (mibayer_submit drains) */
        if (!sh->ring.empty () && sh->ring.back () == f)
          sh->ring.pop_back ();
        if (device_failure (rc)) {
          f->state = F_REDO;
          helper_give_up (sh, mibayer_last_hip_error (), rc == MIBAYER_ERR_TIMEOUT);
        } else {
          f->state = F_FAILED;
          sh->cv_done.notify_all ();
        }
      }
      continue;
    }
    if (!sh->ring.empty ()) {
      Frame *f = sh->ring.front ();
      lk.unlock ();
      int rc = mibayer_wait (sh->ctx, NULL);
      if (rc == MIBAYER_OK && sh->fault_due ())
        rc = MIBAYER_ERR_HIP;
      std::vector<mibayer_stats_zone> zones;
      if (rc == MIBAYER_OK)
        read_stats (sh, f->grid.get (), &zones);
      lk.lock ();
      if (sh->ring.empty () || sh->ring.front () != f)
        continue;               /* the shard was given up meanwhile */
      if (rc == MIBAYER_OK) {
        f->zones.swap (zones);
        sh->ring.pop_front ();
        f->state = F_DONE;
        sh->cv_done.notify_all ();
      } else if (device_failure (rc)) {
        f->rc = rc;
        /* f and everything behind it: F_REDO -- after a deadline, what the context holds: F_LOST */
        helper_give_up (sh, mibayer_last_hip_error (), rc == MIBAYER_ERR_TIMEOUT);
      } else {
        sh->ring.pop_front ();
        f->rc = rc;
        f->state = F_FAILED;
        sh->cv_done.notify_all ();
      }
    }
  }
}

}  /* namespace */

struct mibayer_pool {
  std::vector<Shard *> shards;
  std::deque<Frame> fifo;       /* submission order; element addresses are stable */
  int per_shard = 2;            /* stream.inflight */
  size_t rr = 0;                /* shard whose turn it is */
  size_t redo_rr = 0;
  bool use_helpers = true;      /* MIBAYER_POOL_HELPERS=0: pageable frames on the calling thread */
  bool numa_route = false;      /* the shards' devices span more than one NUMA node */
  bool inverse = false;         /* MIBAYER_FLAG_RGB2BAYER: the source is the 4 B/px side.  A deep context
                                   (MIBAYER_FLAG_SRC_BITS / _DST_16BIT) keeps the destination as the big side:
                                   4 or 8 B/px out against at most 2 B/px in */
  std::unordered_map<const void *, int> node_of;        /* NUMA node of buffers seen so far (pools recycle them) */
  /* frames lost on a device that ran into the wait deadline: their buffers are the device's until it settles */
  struct Lost { void *tag; int shard; };
  std::vector<Lost> lost;
  /* MIBAYER_FLAG_COLOUR: the stage of the frames submitted from now on (NULL: not a colour pool); only the
   * caller's thread touches it, the frames carry their own reference */
  std::shared_ptr<const mibayer_colour> colour;
  /* mibayer_pool_set_stats: the grid of the frames submitted from now on (NULL: off), and the zones of the frame
   * mibayer_pool_wait handed back last (has_zones: it had any) */
  std::shared_ptr<const StatsGrid> grid;
  std::vector<mibayer_stats_zone> last_zones;
  bool has_zones = false;
  std::shared_ptr<const StatsGrid> last_grid;   /* ... which says what last_zones holds */
  std::shared_ptr<const ShadeSet> shade;        /* mibayer_pool_set_shading: the table of the frames submitted from now on */
  std::shared_ptr<const DpcAsk> dpc;            /* mibayer_pool_set_dpc: likewise */
  std::shared_ptr<const mibayer_nr> nr;         /* mibayer_pool_set_nr: likewise */
  /* failure report */
  int unreported = 0;
  int failed_device = -1;
  char failure_msg[320] = "";
};

static int alive_count (const mibayer_pool *pool)
{
  int n = 0;
  for (const Shard *s : pool->shards)
    n += s->alive ? 1 : 0;
  return n;
}

/* Drop shard `idx` from the rotation.  What it had not been given yet is converted on the others; what its context
 * already held is converted again too IF the context could be quiesced (mibayer_internal_abandon: its copies have
 * completed or its queues are dead).  After a wait deadline it cannot: the device may only be slow, its queued
 * uploads may still read those frames' sources and its downloads write their destinations later -- they are LOST
 * (handed back with MIBAYER_ERR_TIMEOUT, buffers quarantined until mibayer_pool_reclaim). */
static void kill_shard (mibayer_pool *pool, int idx, int rc, const char *why)
{
  Shard *sh = pool->shards[(size_t) idx];
  if (!sh->alive)
    return;
  sh->alive = false;
  char reason[200];
  {
    std::lock_guard<std::mutex> lk (sh->mu);
    snprintf (reason, sizeof reason, "%s", (why && why[0]) ? why : sh->errmsg);
    why = reason;
    sh->broken = true;
    if (rc == MIBAYER_ERR_TIMEOUT)
      sh->timed_out = true;
    for (Frame *f : sh->ring)
      f->state = F_REDO;
    sh->ring.clear ();
    for (Frame *f : sh->jobs)
      f->state = F_REDO;
    sh->jobs.clear ();
    sh->cv_job.notify_all ();
  }
  for (Frame &f : pool->fifo)
    if (f.shard == idx && f.state == F_DIRECT)
      f.state = F_REDO;
  /* after this nothing of that context touches the callers' buffers any more -- or the frames it held are lost */
  const bool held = mibayer_internal_abandon (sh->ctx) != MIBAYER_OK;
  int nlost = 0;
  {
    std::lock_guard<std::mutex> lk (sh->mu);
    for (Frame &f : pool->fifo)
      if (f.shard == idx && f.submitted && (f.state == F_REDO || f.state == F_LOST)) {
        nlost += (held && f.state == F_REDO) ? 1 : 0;
        f.state = held ? F_LOST : F_REDO;
      }
    nlost += held ? sh->helper_lost : 0;
    sh->cv_done.notify_all ();
  }
  pool->unreported++;
  pool->failed_device = sh->device;
  char lost_note[64] = "";
  if (nlost > 0)
    snprintf (lost_note, sizeof lost_note, "; %d frame(s) in flight on it lost", nlost);
  snprintf (pool->failure_msg, sizeof pool->failure_msg,
      "shard %d (HIP device %d) dropped from the rotation: %.60s%s%.120s%s; %d device(s) left",
      idx, sh->device, mibayer_strerror (rc), why && why[0] ? " -- " : "",
      why ? why : "", lost_note, alive_count (pool));
}

/* the helper thread of a live shard has seen a device error that the streaming
 * thread has not come across yet (the failed frame sits further back in the
 * queue): take the shard out now, or re-done frames would bounce off it forever */
static bool reap_if_broken (mibayer_pool *pool, int idx)
{
  Shard *sh = pool->shards[(size_t) idx];
  bool broken, timed_out;
  {
    std::lock_guard<std::mutex> lk (sh->mu);
    broken = sh->broken;
    timed_out = sh->timed_out;
  }
  if (broken && sh->alive)
    kill_shard (pool, idx, timed_out ? MIBAYER_ERR_TIMEOUT : MIBAYER_ERR_HIP, NULL);
  return broken;
}

static void start_helper (Shard *sh)
{
  if (!sh->th_started) {
    sh->th = std::thread (helper_main, sh);
    sh->th_started = true;
  }
}

static void queue_to_helper (Shard *sh, Frame *f)
{
  start_helper (sh);
  std::lock_guard<std::mutex> lk (sh->mu);
  f->state = F_QUEUED;
  sh->jobs.push_back (f);
  sh->cv_job.notify_one ();
}

/* The first pageable frame of a shard: from now on its helper thread is the only
 * one that touches the context's submit / wait ring.  Frames the streaming
 * thread had submitted itself and that are still in that ring are handed over,
 * in order, so the helper retires them first. */
static void enter_helper_mode (mibayer_pool *pool, int idx, bool pageable)
{
  Shard *sh = pool->shards[(size_t) idx];
  /* blocking (pageable) copies must not queue behind the other shards' (mibayer_hooks.h); pinned frames keep the
   * shared queues, where their copies go back to back */
  if (sh->helper_mode)
    return;                     /* its thread already drives the context: the queues stay as they are */
  if (pageable)
    mibayer_internal_private_queues (sh->ctx);
  start_helper (sh);
  std::lock_guard<std::mutex> lk (sh->mu);
  sh->helper_mode = true;
  for (Frame &f : pool->fifo)
    if (f.shard == idx && f.state == F_DIRECT) {
      f.state = F_RUNNING;      /* (submitted stays true: the context holds it) */
      sh->ring.push_back (&f);
    }
  sh->cv_job.notify_one ();
}

extern "C" int mibayer_pool_create (const mibayer_pool_cfg *cfg,
    mibayer_pool **out)
{
  if (!out)
    return MIBAYER_ERR_ARG;
  *out = NULL;
  if (!cfg || cfg->struct_size != sizeof (mibayer_pool_cfg))
    return MIBAYER_ERR_ARG;
  if (cfg->ndevices < 1 || cfg->ndevices > MIBAYER_MAX_SHARDS)
    return MIBAYER_ERR_ARG;
  mibayer_pool *pool = new (std::nothrow) mibayer_pool ();
  if (!pool)
    return MIBAYER_ERR_NOMEM;
  for (int i = 0; i < cfg->ndevices; i++) {
    mibayer_cfg one = cfg->stream;
    one.device = cfg->devices[i];
    if (one.device < 0) {
      mibayer_pool_destroy (pool);
      return MIBAYER_ERR_NO_DEVICE;
    }
    mibayer_ctx *c = NULL;
    int rc = mibayer_create (&one, &c);
    if (rc != MIBAYER_OK) {
      mibayer_pool_destroy (pool);
      return rc;
    }
    Shard *sh = new (std::nothrow) Shard ();
    if (!sh) {
      mibayer_destroy (c);
      mibayer_pool_destroy (pool);
      return MIBAYER_ERR_NOMEM;
    }
    sh->ctx = c;
    sh->device = one.device;
    pool->shards.push_back (sh);
  }
  {
    mibayer_cfg resolved;
    if (mibayer_get_cfg (pool->shards[0]->ctx, &resolved) == MIBAYER_OK
        && resolved.inflight > 0)
      pool->per_shard = resolved.inflight;
    for (Shard *sh : pool->shards)
      sh->ring_room = pool->per_shard;
  }
  /* More than one shard: whenever a frame is waited for, the other shards hold queued work, so no wait ever needs to
   * spin for latency's sake (mibayer_set_wait_spin; a context on its own cannot know that its neighbours are busy).
   * MIBAYER_WAIT_SPIN_US in the environment still decides. */
  if (pool->shards.size () > 1 && getenv ("MIBAYER_WAIT_SPIN_US") == NULL)
    for (Shard *sh : pool->shards)
      (void) mibayer_set_wait_spin (sh->ctx, 0);
  /* one shard: a helper would only add a hand-off */
  pool->use_helpers = pool->shards.size () > 1;
  if (const char *e = getenv ("MIBAYER_POOL_HELPERS"))
    pool->use_helpers = atoi (e) != 0;
  pool->inverse = (cfg->stream.flags & MIBAYER_FLAG_RGB2BAYER) != 0;
  if ((cfg->stream.flags & MIBAYER_FLAG_COLOUR) && mibayer_get_colour) {
    /* what the new contexts hold (the identity): frames submitted before any mibayer_pool_set_colour carry it, so a
     * redo on a shard that has moved on since still converts them as they were submitted */
    mibayer_colour first;
    if (mibayer_get_colour (pool->shards[0]->ctx, &first) == MIBAYER_OK) {
      pool->colour = std::make_shared<const mibayer_colour> (first);
      for (Shard *sh : pool->shards)
        sh->applied = pool->colour;
    }
  }
  {
    int first = -2;
    for (Shard *sh : pool->shards) {
      sh->node = mibayer_device_numa_node (sh->device);
      if (sh->node >= 0 && first == -2)
        first = sh->node;
      else if (sh->node >= 0 && sh->node != first)
        pool->numa_route = true;
    }
    if (const char *e = getenv ("MIBAYER_POOL_NUMA"))
      pool->numa_route = pool->numa_route && atoi (e) != 0;
  }
  /* A submit thread per shard, pinned frames included (include/mibayer.h).  Measured (profiles/r04_host_cpu.log,
   * bench.py host_path.host_cpu): queueing a 4K frame from PINNED buffers costs the calling thread 14 us of CPU at the
   * ABI and ~80 us in the element (buffer maps, pool traffic), waiting for it ~8-20 us (napping waits) -- one
   * streaming thread saturates at roughly 11 k frames/s, which is what EIGHT PCIe links carry (8 x ~1.4 k frames/s
   * at 4K).  So pools over six or more DISTINCT GPUs start with a thread per shard (each then spends ~12 % of a core,
   * pinned next to its GPU); smaller pools keep the enqueue-only streaming thread (and shards that see PAGEABLE
   * buffers, 200-300 us of staging copy per frame, get their helper thread either way).  MIBAYER_POOL_THREADS=0 / 1
   * decides otherwise. */
  {
    size_t distinct = 0;
    for (size_t i = 0; i < pool->shards.size (); i++) {
      bool seen = false;
      for (size_t k = 0; k < i; k++)
        seen = seen || pool->shards[k]->device == pool->shards[i]->device;
      distinct += seen ? 0 : 1;
    }
    bool threads = distinct >= 6;
    if (const char *e = getenv ("MIBAYER_POOL_THREADS"))
      threads = atoi (e) != 0;
    if (threads && pool->shards.size () > 1)
      for (size_t i = 0; i < pool->shards.size (); i++)
        enter_helper_mode (pool, (int) i, false);
  }
  if (const char *e = getenv ("MIBAYER_INJECT_FAULT")) {
    /* "shard:frames[,shard:frames...]" */
    while (*e) {
      char *end = NULL;
      const long s = strtol (e, &end, 10);
      if (end == e || *end != ':')
        break;
      e = end + 1;
      const long long n = strtoll (e, &end, 10);
      if (end == e)
        break;
      (void) mibayer_pool_inject_fault (pool, (int) s, n);
      e = (*end == ',') ? end + 1 : end;
    }
  }
  if (const char *e = getenv ("MIBAYER_INJECT_STALL")) {
    /* "shard:frames:ms[,shard:frames:ms...]" */
    while (*e) {
      char *end = NULL;
      const long s = strtol (e, &end, 10);
      if (end == e || *end != ':')
        break;
      e = end + 1;
      const long long n = strtoll (e, &end, 10);
      if (end == e || *end != ':')
        break;
      e = end + 1;
      const long ms = strtol (e, &end, 10);
      if (end == e)
        break;
      if (s >= 0 && s < (long) pool->shards.size () && n >= 0 && ms > 0) {
        pool->shards[(size_t) s]->stall_after = n;
        pool->shards[(size_t) s]->stall_ms = (int) ms;
      }
      e = (*end == ',') ? end + 1 : end;
    }
  }
  *out = pool;
  return MIBAYER_OK;
}

extern "C" void mibayer_pool_destroy (mibayer_pool *pool)
{
  if (!pool)
    return;
  for (Shard *sh : pool->shards) {
    if (sh->th_started) {
      {
        std::lock_guard<std::mutex> lk (sh->mu);
        sh->quit = true;
        sh->broken = true;      /* queued jobs are not started any more */
        sh->cv_job.notify_all ();
      }
      sh->th.join ();
    }
    mibayer_destroy (sh->ctx);
    delete sh;
  }
  delete pool;
}

extern "C" int mibayer_pool_capacity (const mibayer_pool *pool)
{
  if (!pool)
    return MIBAYER_ERR_ARG;
  return alive_count (pool) * pool->per_shard;
}

extern "C" int mibayer_pool_alive (const mibayer_pool *pool)
{
  return pool ? alive_count (pool) : MIBAYER_ERR_ARG;
}

extern "C" int mibayer_pool_pending (const mibayer_pool *pool)
{
  return pool ? (int) pool->fifo.size () : MIBAYER_ERR_ARG;
}

extern "C" int mibayer_pool_inject_fault (mibayer_pool *pool, int shard,
    long long after_frames)
{
  if (!pool || shard < 0 || shard >= (int) pool->shards.size ())
    return MIBAYER_ERR_ARG;
  Shard *sh = pool->shards[(size_t) shard];
  sh->fail_after.store (after_frames < 0 ? -1
      : sh->completions.load () + after_frames);
  return MIBAYER_OK;
}

extern "C" int mibayer_pool_set_wait_timeout (mibayer_pool *pool, int ms)
{
  if (!pool)
    return MIBAYER_ERR_ARG;
  for (Shard *sh : pool->shards)
    (void) mibayer_set_wait_timeout (sh->ctx, ms);
  return MIBAYER_OK;
}

/* The colour stage of the frames submitted from now on.  Nothing is handed to a context here: the pool keeps the
 * stage, every frame takes a reference when mibayer_pool_submit accepts it, and the thread that later gives the frame
 * to a shard's context -- the caller's, the shard's helper thread, a redo on a surviving shard after a failover -- sets
 * the context's stage first (apply_colour).  So a frame that waits in a helper's queue, or is converted again on
 * another device, keeps the parameters it was submitted with, and no frame sees two. */
extern "C" int mibayer_pool_set_colour (mibayer_pool *pool, const mibayer_colour *colour)
{
  if (!pool || !pool->colour || !mibayer_set_colour || !mibayer_colour_in_range (colour))
    return MIBAYER_ERR_ARG;     /* not a colour pool (or no colour stage in this library), or values out of range */
  pool->colour = std::make_shared<const mibayer_colour> (*colour);
  return MIBAYER_OK;
}

/* The statistics grid of the frames submitted from now on, kept with each frame like the colour stage (apply_stats);
 * the range checks are the context layer's: the grid is tried on the first shard's context -- whose own frames carry
 * theirs, and get it back before they are handed over -- so a bad one is refused here and not frames later.  The three
 * setters end here: `g` is what the frames submitted from now on get (no zones, histogram or focus zones: NULL), and
 * `which` says which part of it is new. */
enum { SET_STATS, SET_HIST, SET_FOCUS };
static int pool_set_grid (mibayer_pool *pool, const StatsGrid &g, int which)
{
  const bool hist_call = which == SET_HIST;
  if (g.zones_x == 0 && g.zones_y == 0 && !g.hist && g.fzones_x == 0 && g.fzones_y == 0) {
    pool->grid.reset ();
    return MIBAYER_OK;
  }
  Shard *probe = NULL;
  for (Shard *sh : pool->shards)
    if (sh->alive && !sh->helper_mode) {
      probe = sh;
      break;
    }
  if (probe) {
    const int rc = hist_call ? mibayer_set_hist (probe->ctx, g.hist, g.x0, g.y0, g.w, g.h)
        : which == SET_FOCUS ? mibayer_set_focus (probe->ctx, g.fzones_x, g.fzones_y, g.thr)
        : mibayer_set_stats (probe->ctx, g.zones_x, g.zones_y, g.lo, g.hi);
    if (rc != MIBAYER_OK)
      return rc;
    pool->grid = std::make_shared<const StatsGrid> (g);
    probe->applied_grid = std::make_shared<const StatsGrid> (g);        /* no frame's: apply_stats sets every part */
    return MIBAYER_OK;
  }
  /* every context is driven by a helper thread: the same rule on the resolved configuration */
  mibayer_cfg f;
  if (mibayer_get_cfg (pool->shards[0]->ctx, &f) != MIBAYER_OK || (f.flags & MIBAYER_FLAG_RGB2BAYER))
    return MIBAYER_ERR_ARG;
  const int bits = (int) ((f.flags & MIBAYER_FLAG_SRC_BITS_MASK) >> 8);
  const uint32_t vmax = bits ? (1u << bits) - 1u : 255u;
  if (which == SET_FOCUS && (g.fzones_x | g.fzones_y) && (g.fzones_x < 1 || g.fzones_x > MIBAYER_STATS_MAX_ZONES
          || g.fzones_y < 1 || g.fzones_y > MIBAYER_STATS_MAX_ZONES || g.fzones_x > f.width / 2
          || g.fzones_y > f.height / 2 || g.thr > 2 * vmax))
    return MIBAYER_ERR_ARG;
  if (which == SET_STATS && (g.zones_x | g.zones_y) && (g.zones_x < 1 || g.zones_x > MIBAYER_STATS_MAX_ZONES || g.zones_y < 1
          || g.zones_y > MIBAYER_STATS_MAX_ZONES || g.zones_x > f.width / 2 || g.zones_y > f.height / 2 || g.lo > g.hi
          || g.hi > vmax))
    return MIBAYER_ERR_ARG;
  const bool whole = !(g.x0 | g.y0 | g.w | g.h);
  if (hist_call && g.hist && !whole && (g.x0 < 0 || g.y0 < 0 || ((g.x0 | g.w) & 1) || g.w < 2 || g.h < 1
          || g.w > f.width - g.x0 || g.h > f.height - g.y0))
    return MIBAYER_ERR_ARG;
  pool->grid = std::make_shared<const StatsGrid> (g);
  return MIBAYER_OK;
}

extern "C" int mibayer_pool_set_stats (mibayer_pool *pool, int zones_x, int zones_y, uint32_t lo, uint32_t hi)
{
  if (!pool || !mibayer_set_stats || !mibayer_frame_stats)
    return MIBAYER_ERR_ARG;
  StatsGrid g = pool->grid ? *pool->grid : StatsGrid ();
  g.zones_x = zones_x;
  g.zones_y = zones_y;
  g.lo = lo;
  g.hi = hi;
  return pool_set_grid (pool, g, SET_STATS);
}

extern "C" int mibayer_pool_frame_stats (mibayer_pool *pool, mibayer_stats_zone *out, int nzones)
{
  if (!pool || !out)
    return MIBAYER_ERR_ARG;
  if (!pool->has_zones || pool->last_grid->zones_x == 0)
    return MIBAYER_ERR_EMPTY;
  if (nzones != pool->last_grid->zones_x * pool->last_grid->zones_y)
    return MIBAYER_ERR_ARG;
  memcpy (out, pool->last_zones.data (), (size_t) nzones * sizeof (mibayer_stats_zone));
  return MIBAYER_OK;
}

/* The histogram window of the frames submitted from now on: kept, applied and fetched with the statistics grid */
extern "C" int mibayer_pool_set_hist (mibayer_pool *pool, int on, int x0, int y0, int w, int h)
{
  if (!pool || !mibayer_set_stats || !mibayer_frame_stats || !mibayer_set_hist || !mibayer_frame_hist)
    return MIBAYER_ERR_ARG;
  StatsGrid g = pool->grid ? *pool->grid : StatsGrid ();
  g.hist = on ? 1 : 0;
  g.x0 = on ? x0 : 0;
  g.y0 = on ? y0 : 0;
  g.w = on ? w : 0;
  g.h = on ? h : 0;
  return pool_set_grid (pool, g, SET_HIST);
}

extern "C" int mibayer_pool_frame_hist (mibayer_pool *pool, mibayer_hist *out)
{
  if (!pool || !out)
    return MIBAYER_ERR_ARG;
  if (!pool->has_zones || !pool->last_grid->hist)
    return MIBAYER_ERR_EMPTY;
  memcpy (out, pool->last_zones.data () + (size_t) pool->last_grid->zones_x * pool->last_grid->zones_y, sizeof *out);
  return MIBAYER_OK;
}

/* The focus grid of the frames submitted from now on: kept, applied and fetched with the statistics grid */
extern "C" int mibayer_pool_set_focus (mibayer_pool *pool, int zones_x, int zones_y, uint32_t thr)
{
  if (!pool || !mibayer_set_stats || !mibayer_frame_stats || !mibayer_set_focus || !mibayer_frame_focus)
    return MIBAYER_ERR_ARG;
  StatsGrid g = pool->grid ? *pool->grid : StatsGrid ();
  const bool on = zones_x != 0 || zones_y != 0;
  g.fzones_x = zones_x;
  g.fzones_y = zones_y;
  g.thr = on ? thr : 0;
  return pool_set_grid (pool, g, SET_FOCUS);
}

extern "C" int mibayer_pool_frame_focus (mibayer_pool *pool, mibayer_focus_zone *out, int nzones)
{
  if (!pool || !out)
    return MIBAYER_ERR_ARG;
  if (!pool->has_zones || pool->last_grid->fzones_x == 0)
    return MIBAYER_ERR_EMPTY;
  if (nzones != pool->last_grid->fzones_x * pool->last_grid->fzones_y)
    return MIBAYER_ERR_ARG;
  const size_t before = (size_t) pool->last_grid->zones_x * pool->last_grid->zones_y
      + (pool->last_grid->hist ? kHistZones : 0);
  memcpy (out, pool->last_zones.data () + before, (size_t) nzones * sizeof (mibayer_focus_zone));
  return MIBAYER_OK;
}

/* The shading table of the frames submitted from now on: kept with each frame and applied like the colour stage
 * (apply_shading).  The rules are the context layer's (include/mibayer.h), restated on the resolved configuration so
 * that a bad table is refused here and not frames later. */
extern "C" int mibayer_pool_set_shading (mibayer_pool *pool, const mibayer_shading *shading)
{
  if (!pool || !mibayer_set_shading)
    return MIBAYER_ERR_ARG;
  if (!shading) {
    pool->shade.reset ();
    return MIBAYER_OK;
  }
  mibayer_cfg f;
  if (mibayer_get_cfg (pool->shards[0]->ctx, &f) != MIBAYER_OK || (f.flags & MIBAYER_FLAG_RGB2BAYER)
      || shading->struct_size != sizeof (mibayer_shading) || !shading->table || shading->cell_log2_x < 2
      || shading->cell_log2_x > 8 || shading->cell_log2_y < 2 || shading->cell_log2_y > 8)
    return MIBAYER_ERR_ARG;
  const int nx = ((f.width - 1) >> shading->cell_log2_x) + 2, ny = ((f.height - 1) >> shading->cell_log2_y) + 2;
  const int bits = (int) ((f.flags & MIBAYER_FLAG_SRC_BITS_MASK) >> 8);
  const uint32_t vmax = bits ? (1u << bits) - 1u : 255u;
  if (nx > MIBAYER_SHADING_MAX_NODES || ny > MIBAYER_SHADING_MAX_NODES)
    return MIBAYER_ERR_ARG;
  for (int s = 0; s < 4; s++)
    if (shading->black[s] > vmax)
      return MIBAYER_ERR_ARG;
  const size_t n = (size_t) 4 * (size_t) ny * (size_t) nx;
  for (size_t e = 0; e < n; e++)
    if (shading->table[e] > 32767)
      return MIBAYER_ERR_ARG;
  auto set = std::make_shared<ShadeSet> ();
  set->table.assign (shading->table, shading->table + n);
  set->par = *shading;
  set->par.table = set->table.data ();
  pool->shade = set;
  return MIBAYER_OK;
}

/* The defective pixel correction of the frames submitted from now on, kept with each frame like the shading table
 * (apply_dpc); the rules are the context layer's (include/mibayer.h), restated on the resolved configuration. */
extern "C" int mibayer_pool_set_dpc (mibayer_pool *pool, const mibayer_dpc *dpc)
{
  if (!pool || !mibayer_set_dpc)
    return MIBAYER_ERR_ARG;
  if (!dpc) {
    pool->dpc.reset ();
    return MIBAYER_OK;
  }
  mibayer_cfg f;
  if (mibayer_get_cfg (pool->shards[0]->ctx, &f) != MIBAYER_OK || (f.flags & MIBAYER_FLAG_RGB2BAYER)
      || dpc->struct_size != sizeof (mibayer_dpc))
    return MIBAYER_ERR_ARG;
  const int bits = (int) ((f.flags & MIBAYER_FLAG_SRC_BITS_MASK) >> 8);
  const int vmax = bits ? (1 << bits) - 1 : 255;
  if (dpc->hot < -1 || dpc->hot > vmax || dpc->cold < -1 || dpc->cold > vmax || dpc->ndefects > MIBAYER_DPC_MAX_DEFECTS
      || (dpc->ndefects > 0 && !dpc->defects))
    return MIBAYER_ERR_ARG;
  for (uint32_t e = 0; e < dpc->ndefects; e++)
    if (dpc->defects[2 * e] >= (uint32_t) f.width || dpc->defects[2 * e + 1] >= (uint32_t) f.height)
      return MIBAYER_ERR_ARG;
  if (f.height < 4)
    return MIBAYER_ERR_GEOMETRY;
  auto set = std::make_shared<DpcAsk> ();
  set->list.assign (dpc->defects, dpc->defects + 2 * (size_t) dpc->ndefects);
  set->par = *dpc;
  set->par.defects = set->list.data ();
  pool->dpc = set;
  return MIBAYER_OK;
}

/* The noise reduction curve of the frames submitted from now on, kept with each frame like the defect pass's parameters
 * (apply_nr); the rules are the context layer's (include/mibayer.h), restated on the resolved configuration. */
extern "C" int mibayer_pool_set_nr (mibayer_pool *pool, const mibayer_nr *nr)
{
  if (!pool || !mibayer_set_nr)
    return MIBAYER_ERR_ARG;
  if (!nr) {
    pool->nr.reset ();
    return MIBAYER_OK;
  }
  mibayer_cfg f;
  if (mibayer_get_cfg (pool->shards[0]->ctx, &f) != MIBAYER_OK || (f.flags & MIBAYER_FLAG_RGB2BAYER)
      || nr->struct_size != sizeof (mibayer_nr))
    return MIBAYER_ERR_ARG;
  const int bits = (int) ((f.flags & MIBAYER_FLAG_SRC_BITS_MASK) >> 8);
  const int vmax = bits ? (1 << bits) - 1 : 255;
  for (int i = 0; i < MIBAYER_NR_NODES; i++)
    if (nr->curve[i] > (vmax < 2047 ? vmax : 2047))
      return MIBAYER_ERR_ARG;
  if (f.width < 6 || f.height < 5)
    return MIBAYER_ERR_GEOMETRY;
  pool->nr = std::make_shared<mibayer_nr> (*nr);
  return MIBAYER_OK;
}

extern "C" int mibayer_pool_inject_stall (mibayer_pool *pool, int shard, int ms)
{
  if (!pool || shard < 0 || shard >= (int) pool->shards.size ())
    return MIBAYER_ERR_ARG;
  return mibayer_internal_stall (pool->shards[(size_t) shard]->ctx, ms);
}

extern "C" int mibayer_pool_take_failure (mibayer_pool *pool, int *device,
    int *alive, char *msg, size_t msg_len)
{
  if (!pool)
    return MIBAYER_ERR_ARG;
  if (pool->unreported == 0)
    return 0;
  const int n = pool->unreported;
  pool->unreported = 0;
  if (device)
    *device = pool->failed_device;
  if (alive)
    *alive = alive_count (pool);
  if (msg && msg_len)
    snprintf (msg, msg_len, "%s", pool->failure_msg);
  return n;
}

extern "C" int mibayer_pool_submit (mibayer_pool *pool, const uint8_t *src,
    uint8_t *dst, void *tag)
{
  if (!pool || !src || !dst)
    return MIBAYER_ERR_ARG;
  const size_t n = pool->shards.size ();
  for (;;) {
    /* the next live shard in rotation */
    size_t idx = n;
    for (size_t k = 0; k < n; k++) {
      const size_t i = (pool->rr + k) % n;
      if (pool->shards[i]->alive) {
        idx = i;
        break;
      }
    }
    if (idx == n)
      return MIBAYER_ERR_HIP;   /* no device left */
    if (reap_if_broken (pool, (int) idx))
      continue;
    const size_t turn = idx;
    if (pool->numa_route) {
      /* the live shard next to the frame's big buffer, if taking it keeps the rotation balanced (the destination
       * of bayer2rgb at every depth: 16-bit samples in, 8 B/px out is still the bigger side) */
      const void *big = pool->inverse ? (const void *) src : (const void *) dst;
      int node;
      auto it = pool->node_of.find (big);
      if (it != pool->node_of.end ()) {
        node = it->second;
      } else {
        node = mibayer_host_numa_node (big);
        if (pool->node_of.size () > 4096)
          pool->node_of.clear ();
        pool->node_of.emplace (big, node);
      }
      if (node >= 0 && pool->shards[turn]->node != node) {
        for (size_t k = 1; k < n; k++) {
          const size_t i = (turn + k) % n;
          Shard *cand = pool->shards[i];
          if (cand->alive && cand->node == node && cand->inflight < pool->per_shard
              && cand->assigned < pool->shards[turn]->assigned + pool->per_shard) {
            bool broken;
            {
              std::lock_guard<std::mutex> lk (cand->mu);
              broken = cand->broken;
            }
            if (!broken) {
              idx = i;
              break;
            }
          }
        }
      }
    }
    Shard *sh = pool->shards[idx];
    if (sh->inflight >= pool->per_shard)
      return MIBAYER_ERR_BUSY;
    if (sh->stall_ms > 0 && sh->assigned >= sh->stall_after) {  /* drill: MIBAYER_INJECT_STALL */
      const int ms = sh->stall_ms;
      sh->stall_ms = 0;
      (void) mibayer_internal_stall (sh->ctx, ms);
    }
    Frame f = { src, dst, tag, (int) idx, (int) idx, F_DIRECT, MIBAYER_OK, false, pool->colour, pool->grid, {}, pool->shade, pool->dpc, pool->nr };
    if (pool->use_helpers && (mibayer_internal_is_pageable (src) || mibayer_internal_is_pageable (dst))
        && !sh->pageable_seen) {
      sh->pageable_seen = true;
      enter_helper_mode (pool, (int) idx, true);
    }
    if (sh->helper_mode) {
      pool->fifo.push_back (f);
      queue_to_helper (sh, &pool->fifo.back ());
    } else {
      apply_colour (sh, &f);
      apply_stats (sh, &f);
      const int rc = mibayer_submit (sh->ctx, src, dst, tag);
      if (device_failure (rc)) {
        kill_shard (pool, (int) idx, rc, mibayer_last_hip_error ());
        continue;               /* this frame goes to the next live shard */
      }
      if (rc != MIBAYER_OK)
        return rc;
      f.submitted = true;
      pool->fifo.push_back (f);
    }
    sh->inflight++;
    sh->assigned++;
    if (idx == turn)
      pool->rr = (idx + 1) % n;
    return MIBAYER_OK;
  }
}

extern "C" int mibayer_pool_wait (mibayer_pool *pool, void **tag)
{
  if (!pool)
    return MIBAYER_ERR_ARG;
  if (pool->fifo.empty ())
    return MIBAYER_ERR_EMPTY;
  Frame &f = pool->fifo.front ();
  const size_t n = pool->shards.size ();
  for (;;) {
    Shard *sh = pool->shards[(size_t) f.shard];
    int state;
    {
      std::unique_lock<std::mutex> lk (sh->mu);
      sh->cv_done.wait (lk, [&f] {
        return f.state != F_QUEUED && f.state != F_RUNNING;
      });
      state = f.state;
    }
    if (state == F_DONE)
      break;
    if (state == F_DIRECT) {
      int rc = mibayer_wait (sh->ctx, NULL);
      if (rc == MIBAYER_OK && sh->fault_due ())
        rc = MIBAYER_ERR_HIP;
      if (rc == MIBAYER_OK) {
        fetch_stats (sh, &f);
        break;
      }
      if (!device_failure (rc))
        return rc;
      kill_shard (pool, f.shard, rc, mibayer_last_hip_error ());    /* f becomes F_REDO */
      continue;
    }
    if (state == F_FAILED)
      return f.rc;              /* not a device failure (those become F_REDO): the caller's to handle */
    if (state == F_LOST) {
      /* The helper thread may have marked it while the shard still counts as alive to this thread: take the shard
       * out first, so that mibayer_pool_alive() / take_failure already tell the caller what happened
       * when the lost frame comes back, and kill_shard() has its last word on held-vs-quiesced (a context that
       * could be quiesced after all turns the frame into F_REDO: converted elsewhere instead of lost). */
      (void) reap_if_broken (pool, f.shard);
      {
        std::lock_guard<std::mutex> lk (sh->mu);
        state = f.state;
      }
      if (state != F_LOST)
        continue;
      /* in flight on a device that ran into the deadline: handed back as lost, in order; its buffers stay the
       * device's until mibayer_pool_reclaim() says otherwise */
      pool->lost.push_back (mibayer_pool::Lost { f.tag, f.shard });
      pool->has_zones = false;
      pool->last_zones.clear ();
      if (tag)
        *tag = f.tag;
      pool->shards[(size_t) f.owner]->inflight--;
      pool->fifo.pop_front ();
      return MIBAYER_ERR_TIMEOUT;
    }
    /* F_REDO: once more on a device that is still in the rotation.  First the shard it came from: if its helper
     * thread saw the failure, the shard is still "alive" to this thread and its context still has the frame's
     * copies queued -- take it out and abandon it BEFORE the frame is converted elsewhere and handed back, or a late
     * DMA of the dead context lands in a buffer the caller has already released. */
    (void) reap_if_broken (pool, f.shard);
    {
      std::lock_guard<std::mutex> lk (sh->mu);
      if (f.state == F_LOST)    /* the quiesce ran into the deadline: not converted again after all */
        continue;
    }
    size_t idx = n;
    for (size_t k = 0; k < n; k++) {
      const size_t i = (pool->redo_rr + k) % n;
      if (pool->shards[i]->alive) {
        idx = i;
        break;
      }
    }
    if (idx == n)
      return MIBAYER_ERR_HIP;   /* no device left: the stream has failed */
    if (reap_if_broken (pool, (int) idx))
      continue;
    pool->redo_rr = (idx + 1) % n;
    Shard *to = pool->shards[idx];
    f.shard = (int) idx;
    f.submitted = false;
    if (to->helper_mode) {
      /* its helper thread owns the context: an ordinary job for it */
      queue_to_helper (to, &f);
      continue;
    }
    f.submitted = true;         /* while the spare slot of `to` works on it */
    f.state = F_REDO;
    apply_colour (to, &f);
    apply_stats (to, &f);
    int rc = mibayer_internal_run_spare (to->ctx, f.src, f.dst);
    if (rc == MIBAYER_OK && to->fault_due ())
      rc = MIBAYER_ERR_HIP;
    if (rc == MIBAYER_OK) {
      fetch_stats (to, &f);
      break;
    }
    if (!device_failure (rc))
      return rc;
    kill_shard (pool, (int) idx, rc, mibayer_last_hip_error ());       /* F_REDO again, or F_LOST after a deadline */
  }
  if (tag)
    *tag = f.tag;
  pool->has_zones = f.grid && !f.zones.empty ();
  pool->last_grid = f.grid;
  pool->last_zones.swap (f.zones);
  pool->shards[(size_t) f.owner]->inflight--;
  pool->fifo.pop_front ();
  return MIBAYER_OK;
}

extern "C" int mibayer_pool_lost (const mibayer_pool *pool)
{
  return pool ? (int) pool->lost.size () : MIBAYER_ERR_ARG;
}

extern "C" int mibayer_pool_reclaim (mibayer_pool *pool, void **tag)
{
  if (!pool)
    return MIBAYER_ERR_ARG;
  for (size_t i = 0; i < pool->lost.size (); i++) {
    const mibayer_pool::Lost l = pool->lost[i];
    if (mibayer_internal_settled (pool->shards[(size_t) l.shard]->ctx)) {
      if (tag)
        *tag = l.tag;
      pool->lost.erase (pool->lost.begin () + (long) i);
      return MIBAYER_OK;
    }
  }
  return MIBAYER_ERR_EMPTY;
}

extern "C" int mibayer_pool_set_wait_spin (mibayer_pool *pool, int spin_us)
{
  if (!pool)
    return MIBAYER_ERR_ARG;
  for (Shard *sh : pool->shards)
    (void) mibayer_set_wait_spin (sh->ctx, spin_us);
  return MIBAYER_OK;
}

extern "C" int mibayer_pool_get_host_stats (const mibayer_pool *pool, mibayer_host_stats *out)
{
  if (!pool || !out)
    return MIBAYER_ERR_ARG;
  memset (out, 0, sizeof *out);
  for (const Shard *sh : pool->shards) {
    mibayer_host_stats one;
    if (mibayer_get_host_stats (sh->ctx, &one) != MIBAYER_OK)
      continue;
    out->submits += one.submits;
    out->waits += one.waits;
    out->polls += one.polls;
    out->naps += one.naps;
    out->submit_cpu_ms += one.submit_cpu_ms;
    out->wait_cpu_ms += one.wait_cpu_ms;
    out->wait_wall_ms += one.wait_wall_ms;
  }
  return MIBAYER_OK;
}
