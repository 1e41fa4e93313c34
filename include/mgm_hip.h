/*
 * mgm_hip.h -- C ABI of libmgm_hip.so, the MI355X (gfx950) MGM stereo core.
 *
 * This is the drop-in boundary for the hot path of gfacciol/mgm:
 *
 *   allocate_and_fill_sgm_costvolume()  mgm_costvolume.h:337-424   -> mgm_costvolume_build[_dev]
 *   compute_mgm_weights()               mgm_weights.h:63-85        -> mgm_weights[_dev]
 *   mgm()                               mgm_core.cc:408-613        -> mgm_aggregate[_dev]
 *   subpixel_refinement_sgm()           mgm_refine.h:40-70         -> mgm_refine[_dev]
 *
 * which the reference's main() calls at mgm.cc:372-385 (and again for the
 * right-to-left run at mgm.cc:405-414).  INTEGRATION.md shows the replacement
 * of those call sites.
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, ints; every function returns an
 *     mgm_status (0 = MGM_OK) and never throws or aborts across the boundary;
 *     mgm_last_error(ctx) gives the text of the last failure on that context.
 *     A call that fails hands out nothing it created: an output handle is
 *     either not written at all or reset to NULL, never left pointing at a
 *     half-made object (a volume passed in to be refilled stays the caller's).
 *   - images are the reference's `struct Img` layout (img.h:35-51): planar
 *     float32, data[x + y*nx + c*nx*ny].
 *   - cost volumes are the reference's per-pixel `Dvec` order (dvec.cc:49-131)
 *     made dense: float32 [y][x][o], o = 0..L-1 <-> disparity dmin+o,
 *     L = dmax-dmin+1 (dvec.cc:60).  Reads outside [dmin,dmax] behave as +INF.
 *   - weights are 8 planes in the order W,E,S,N,NW,NE,SE,SW (mgm_weights.h:69).
 *   - one mgm_ctx per host thread; a ctx is bound to one device and owns one
 *     HIP stream.  The *_dev entry points enqueue on that stream and return
 *     without synchronising (results are ordered on the stream); entry points
 *     that take or return HOST buffers synchronise before returning.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute
 *     entry point fails with MGM_ERR_HIP.
 */
#ifndef MGM_HIP_H_
#define MGM_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgm_ctx mgm_ctx; /* device + stream + workspace */
typedef struct mgm_img mgm_img; /* device-resident planar float image */
typedef struct mgm_cv mgm_cv;   /* device-resident dense volume [ny][nx][L] */

typedef enum mgm_status {
    MGM_OK = 0,
    MGM_ERR_INVALID = 1,     /* bad argument */
    MGM_ERR_UNSUPPORTED = 2, /* valid in the reference, not built yet */
    MGM_ERR_HIP = 3,         /* HIP runtime error / no device */
    MGM_ERR_NOMEM = 4,
    MGM_ERR_INTERNAL = 5     /* in-kernel watchdog fired (dataflow hand-off timed out) */
} mgm_status;

/* ---- context ---------------------------------------------------------- */
/* MGM_ERR_HIP if `device` does not exist or is not a gfx950 part. */
int mgm_ctx_create(int device, mgm_ctx **ctx);
int mgm_ctx_destroy(mgm_ctx *ctx);
const char *mgm_last_error(const mgm_ctx *ctx);
int mgm_ctx_synchronize(mgm_ctx *ctx);
/* Hand the context's grow-only workspace (Lr volumes of the largest aggregation so far, hand-off slots, ...) back to the
 * device; it is allocated again on demand.  Synchronises. */
int mgm_ctx_trim(mgm_ctx *ctx);
/* Cap, in bytes, on the workspace ONE pass launch may take (the NDIR Lr volumes of every batched volume and the
 * hand-off slots; 0 = no cap, the default).  mgm_aggregate_batch_dev runs a batch that exceeds it -- or that the
 * device cannot hold -- as several launches over the largest sub-batches that fit instead of returning MGM_ERR_NOMEM. */
int mgm_ctx_set_workspace_limit(mgm_ctx *ctx, unsigned long long bytes);
/* PIPELINED CONTEXT for a caller that has ONE volume (or one small batch) at a time -- a stream of stereo pairs.
 * depth 1 (the default): every call runs when it is made.  depth D = 2..16: mgm_aggregate[_batch]_dev calls are DEFERRED --
 * checked, remembered, MGM_OK returned -- until D of them have been gathered, and those then run as ONE batch: one launch
 * of the pass kernel over all their volumes (what mgm_aggregate_batch_dev does for a caller that has the volumes
 * together: a single volume's launch is bound by its chains of bands, and the other volumes' bands fill its gaps; round
 * 4, 1920x1080x256, 8 directions, FH: 0.70 of the roofline one volume at a time, 0.82 with D = 2, 0.87 with D = 4).  Every
 * volume gets exactly the result of an unpipelined call.  The workspace holds the Lr volumes of D calls.
 * What the caller must know: (1) results exist once the D-th call of a group, mgm_ctx_synchronize or any other entry point
 * of the context that is not part of gathering a step has returned (downloads, post-processing, frees and the rest first
 * run what has been deferred); (2) consecutive calls need DIFFERENT cost volumes, weight images and output images (D sets,
 * used in turn) -- refilling a volume or weights that a deferred call still needs, or naming an output image twice, is
 * still correct (the deferred calls then run first) but defeats the gathering; (3) an error of the deferred work is
 * returned by the call that made it run.  A call that does not fit the waiting ones (other geometry or settings, S
 * wanted) makes them run first.  Synchronises; MGM_ERR_INVALID for a depth outside 1..16. */
int mgm_ctx_set_pipeline(mgm_ctx *ctx, int depth);
/* PLACEMENT of the Lr workspace.  Identical launches run on plateaus up to 16 % apart depending on which physical pages the
 * allocator handed out for the workspace (docs/experiments.md, rounds 4 and 5: same code, data and virtual address).  With
 * tries = n >= 2 the context, whenever an aggregation has just (re)allocated its workspace, times that aggregation's pass
 * launch on up to n allocations -- the earlier ones held meanwhile, so that each lands on other pages -- and keeps the
 * fastest.  Results do not change (the launch is simply repeated on the same inputs); the first aggregation after a
 * (re)allocation takes n - 1 allocations and 2 n - 1 launches longer, and needs room for two workspaces (skipped when the
 * device does not have it).  0 (default) / 1: take what the allocator gives.  For long-lived contexts (resident mode,
 * services, benchmarks); a one-shot command line would pay more than it gains. */
int mgm_ctx_set_placement_tries(mgm_ctx *ctx, int tries);
/* Free and total device memory in bytes as the runtime sees them now (hipMemGetInfo on the context's device): what a
 * caller sizes its batches -- or mgm_ctx_set_workspace_limit -- with.  Either pointer may be NULL. */
int mgm_ctx_mem_info(mgm_ctx *ctx, unsigned long long *free_bytes, unsigned long long *total_bytes);
void *mgm_ctx_stream(mgm_ctx *ctx); /* the hipStream_t everything is enqueued on */
const char *mgm_version(void);

/* Per-kernel timing with HIP events on the ctx stream.  While enabled every
 * kernel launch is bracketed by an event pair; mgm_timing_get() synchronises
 * and reports elapsed milliseconds per launch in launch order.  A cost-volume
 * fill is listed TWICE with the same milliseconds: as "k_cost", then under the
 * name of the kernel the dispatcher chose ("k_cost_diffx_1b", "k_cost_ncc",
 * "k_cost_general", ...): sum the table by name, not over all of its rows. */
int mgm_timing_enable(mgm_ctx *ctx, int enable);
int mgm_timing_reset(mgm_ctx *ctx);
int mgm_timing_count(mgm_ctx *ctx);
int mgm_timing_get(mgm_ctx *ctx, int idx, const char **kernel_name, float *ms);

/* ---- images (struct Img, img.h:9-59) ----------------------------------- */
int mgm_img_create(mgm_ctx *ctx, int nx, int ny, int nch, mgm_img **img);
int mgm_img_upload(mgm_ctx *ctx, const float *host, int nx, int ny, int nch, mgm_img **img);
/* Refill an existing image from a host buffer of its own size (no allocation; synchronises, so the buffer is the caller's
 * again on return): a caller with a stream of same-sized inputs keeps its device images (src/mgm_main.cc, resident mode). */
int mgm_img_update(mgm_ctx *ctx, mgm_img *img, const float *host);
int mgm_img_download(mgm_ctx *ctx, const mgm_img *img, float *host);
int mgm_img_dims(const mgm_img *img, int *nx, int *ny, int *nch);
/* The raw device pointer.  Does NOT synchronise and does NOT run deferred work: on a pipelined context
 * (mgm_ctx_set_pipeline) call mgm_ctx_synchronize first if the image is an output of a deferred aggregation. */
void *mgm_img_device_ptr(mgm_img *img);
int mgm_img_device(const mgm_img *img); /* HIP device ordinal the pixels live on (-1: NULL) */
int mgm_img_free(mgm_ctx *ctx, mgm_img *img);

/* ---- volumes (costvolume_t, mgm_costvolume.h:311-327) ------------------ */
int mgm_cv_create(mgm_ctx *ctx, int nx, int ny, int dmin, int dmax, mgm_cv **cv);
int mgm_cv_upload(mgm_ctx *ctx, const float *dense, int nx, int ny, int dmin, int dmax, mgm_cv **cv);
int mgm_cv_download(mgm_ctx *ctx, const mgm_cv *cv, float *dense);
int mgm_cv_dims(const mgm_cv *cv, int *nx, int *ny, int *dmin, int *dmax);
void *mgm_cv_device_ptr(mgm_cv *cv);
int mgm_cv_device(const mgm_cv *cv); /* HIP device ordinal of the context that made the volume (-1: NULL) */
int mgm_cv_free(mgm_ctx *ctx, mgm_cv *cv);

/* ---- cost volume: allocate_and_fill_sgm_costvolume --------------------- */
/* prefilter in {"none","census","sobelx","gblur"}, distance in {"ad","sd","census",
 * "ncc","btad","btsd"}; unknown names silently select the first entry, as the
 * reference does (mgm_costvolume.h:184-190, 201-207).  census_win is the value
 * of the reference's CENSUS_NCC_WIN environment parameter (mgm_costvolume.h:61).
 * Every entry of both tables is built on the device.  *C must be NULL (a new volume is allocated) or a volume of
 * the same geometry, which is then refilled in place (no allocation, no sync). */
int mgm_costvolume_build_dev(mgm_ctx *ctx, const mgm_img *u, const mgm_img *v, int dmin, int dmax,
                             const char *prefilter, const char *distance, float truncDist, int census_win,
                             mgm_cv **C);
/* Host-buffer form taking the reference's per-pixel range images (dminI/dmaxI, mgm.cc:338-353), converted to
 * int as Dvec's constructor does (mgm_costvolume.h:323).  Uniform ranges take the fast path.  RAGGED ranges
 * (-m/-M files) give a volume over the hull of all ranges in which a pixel only owns the disparities of its own
 * range -- the others read +INF, as Dvec::operator[] does (dvec.cc:129), and are exempt from the "no finite cost"
 * rule; mgm_aggregate* then searches the winner and gates the refinement inside each pixel's range.  The hull may
 * span any number of labels the device can hold (the reference's Dvec has no limit, dvec.cc:60; an index-arithmetic cap of
 * 4 194 304 aside): up to 1024 on the fast kernels, up to 2048 on the first build of the pass kernel, beyond that on the
 * generic ones (a second or more per full-HD volume); batched ragged volumes must share hull_min under FH potentials.
 * A ragged volume whose windows are at most 126 labels wide also keeps a RANGE-PROPORTIONAL copy (64 or 128 label slots per pixel at
 * the pixel's own window, mgm_costvolume.h:275-299), which mgm_aggregate* then walks instead of the hull: same results, bytes and
 * steps proportional to the labels that exist. */
int mgm_costvolume_build(mgm_ctx *ctx, const float *u, const float *v, int nx, int ny, int nch, int vnx, int vny,
                         const float *dminI, const float *dmaxI, const char *prefilter, const char *distance,
                         float truncDist, int census_win, mgm_cv **C);

/* Device form of the ragged build: dminI/dmaxI are nx*ny device images, [hull_min, hull_max] must contain every
 * pixel's (int) range. */
int mgm_costvolume_build_ranged_dev(mgm_ctx *ctx, const mgm_img *u, const mgm_img *v, const mgm_img *dminI,
                                    const mgm_img *dmaxI, int hull_min, int hull_max, const char *prefilter,
                                    const char *distance, float truncDist, int census_win, mgm_cv **C);

/* ---- sub-pixel label spacing: half- and quarter-pixel cost volumes (DESIGN.md "sub-pixel labels"; this library's own mode) ----
 * The other image is matched at the fractional shifts k/s, k = 0..s-1, s = 1, 2 or 4: s phase images v_k, s ordinary builds C_k over
 * [dmin, dmax], interleaved into ONE fine volume F with the labels s*dmin .. s*dmax, s*(dmax-dmin)+1 of them; fine label d' stands
 * for the disparity d'/s.
 *   phase image  v_0 is v, the same bits.  k > 0, t = k/s, per channel and row in fp32, column indices clamped to [0, vnx-1], every
 *                product rounded and the sums in the order written (no contraction), non-finite pixels as IEEE gives:
 *                  "linear"  v_k(x) = (1-t)*v(x) + t*v(x+1)
 *                  "cubic"   v_k(x) = ((w0*v(x-1) + w1*v(x)) + w2*v(x+1)) + w3*v(x+2), Keys' weights (a = -1/2), exact in fp32:
 *                            t = 1/4: -9/128, 111/128, 29/128, -3/128;  1/2: -1/16, 9/16, 9/16, -1/16;  3/4: t = 1/4 reversed
 *   fine volume  with o' = d' - s*dmin:  F(y,x,o') = C_{o' mod s}(y,x,o' div s), the same bits, where C_k is exactly what
 *                mgm_costvolume_build_dev(u, v_k, dmin, dmax, ...) produces, its "no finite cost => zeros" rule included; label
 *                dmax of the phases k > 0 is dropped.  s = 1: F is C_0.  With non-finite pixels in v a fractional phase can lose
 *                every label of a pixel where phase 0 keeps some: that phase's entries then read 0 by that rule -- use finite images.
 * mgm_aggregate*, every winner search, the refinements and the runner-up search take F as any dense volume and work per FINE label:
 * their maps are in fine units (mgm_subpix_scale_dev: out = in / (float)s, exact, NaN stays NaN; cost maps are not rescaled), and a
 * slope of one pixel now takes s steps of P1.  The right view is the same call with the images exchanged and [-dmax, -dmin].
 * F leaves the call in the state a direct build of its label count would leave it: one-byte codes (the compact or the padded compact
 * copy, the fp32 copy stale) when every phase holds them by construction -- single-word census -- and an fp32 volume without copies,
 * like an uploaded one, in every other case.  *F / *out: NULL for a new object, or one of the same geometry, refilled in place.
 * Scratch: one phase image and s phase volumes of the [dmin, dmax] geometry, kept by the context for the next call of that geometry
 * (mgm_ctx_trim releases them; like the other steps' scratch they are not part of what mgm_ctx_set_workspace_limit caps).
 * MGM_ERR_INVALID: s outside {1, 2, 4}, k outside 0..s-1, an interp that is neither name, dmax < dmin, images of different channel
 * counts, an object to refill of another geometry (for the phase image also: v itself).  mgm_subpix_scale_dev: out may be in.
 * No synchronisation; the timing table lists k_subpix_phase, k_cv_interleave and k_scale_map. */
int mgm_subpix_phase_dev(mgm_ctx *ctx, const mgm_img *v, int s, int k, const char *interp, mgm_img **out);
int mgm_costvolume_build_subpix_dev(mgm_ctx *ctx, const mgm_img *u, const mgm_img *v, int dmin, int dmax, int s,
                                    const char *interp, const char *prefilter, const char *distance, float truncDist,
                                    int census_win, mgm_cv **F);
int mgm_subpix_scale_dev(mgm_ctx *ctx, const mgm_img *in, int s, mgm_img *out);

/* ---- edge weights: compute_mgm_weights --------------------------------- */
/* compute_mgm_weights (mgm_weights.h:63-85; called at mgm.cc:372 when -aP2 != 1): 8 planes of nx*ny weights.  *w8 == NULL
 * on entry: a new image is created; non-NULL: that nx*ny*8 image is refilled (like *C of mgm_costvolume_build_dev). */
int mgm_weights_dev(mgm_ctx *ctx, const mgm_img *u, float aP, float aThresh, mgm_img **w8);

/* ---- aggregation + WTA: mgm() ------------------------------------------ */
/* C is not modified.  w8 may be NULL (all ones).  A volume whose aggregation can meet NaNs -- NaN costs (an uploaded
 * volume is scanned once per filling; `-p census` with another distance from descriptors of more than 24 bits), or a ragged
 * volume with P2 = +INF (all-INF slabs, then INF - INF) -- is aggregated by a slow kernel that keeps the OPERAND ORDER of
 * the reference's minima (`a < b ? a : b`, mgm_core.cc:48-60; dvec.cc:81-88), which decides what a NaN does there: the
 * results are still the reference's, at a second or so per full-HD volume instead of milliseconds.  As in the reference
 * (mgm_core.cc:420-423) a single weight != 1.0 anywhere switches the whole run
 * to the weighted update functions.  P1/P2 are used as given (the caller has
 * already multiplied by the channel count, mgm.cc:356-357).
 *   NDIR 1..8, MGM (TSGM) 1..4, use_fh: USE_TRUNCATED_LINEAR_POTENTIALS,
 *   fix_overcount: TSGM_FIX_OVERCOUNT.
 * refine: NULL/"none" gives mgm()'s own outputs (integer labels dmin+argmin);
 *   "vfit" additionally applies subpixel_refinement_sgm in the same kernel; "parabola", "cubic" and
 *   "parabolaOCV" apply it as a second kernel on the corrected S.
 * out/outcost: nx*ny images.  S: NULL, or receives the corrected aggregated
 *   volume that mgm() returns (costs one extra volume write). */
int mgm_aggregate_dev(mgm_ctx *ctx, const mgm_cv *C, const mgm_img *w8, float P1, float P2, int NDIR, int MGM,
                      int use_fh, int fix_overcount, const char *refine, mgm_img *out, mgm_img *outcost,
                      mgm_cv **S);
int mgm_aggregate(mgm_ctx *ctx, const mgm_cv *C, const float *w8, float P1, float P2, int NDIR, int MGM, int use_fh,
                  int fix_overcount, const char *refine, float *out, float *outcost, mgm_cv **S);

/* n (1..16) volumes of identical size and label count aggregated by ONE launch of the pass kernel:
 * the two runs of mgm() that main() makes for a stereo pair, left->right (mgm.cc:376-385) and
 * right->left (mgm.cc:405-414), or the volumes of consecutive pairs.  Every volume gets exactly the
 * result mgm_aggregate_dev would give it; the point is throughput -- the scan-line passes of one
 * volume form dependency chains (band after band) that leave compute units waiting, and the other
 * volumes' bands fill those gaps (a throughput-bound launch puts two bands on a compute unit; at 128 / 64
 * labels two / four volumes share every wavefront).  The workspace holds NDIR fp32 volumes per batched volume.  C, out, outcost: arrays of n handles.  w8: NULL, or an array of n
 * weight images (for all volumes or none; all weighted or all unweighted).  S: NULL, or an array of
 * n handles to receive the corrected aggregated volumes. */
int mgm_aggregate_batch_dev(mgm_ctx *ctx, int n, const mgm_cv *const *C, const mgm_img *const *w8, float P1, float P2,
                            int NDIR, int MGM, int use_fh, int fix_overcount, const char *refine, mgm_img *const *out,
                            mgm_img *const *outcost, mgm_cv **S);

/* ---- one volume sharded by DIRECTION over several GPUs ---------
 * Each rank holds the full C (rebuilt from the images: cheaper than broadcasting it) and runs
 * a contiguous subset of the passes; pass first_pass+k's Lr volume stays in workspace slot k
 * (mgm_lr_device_ptr).  The ranks then exchange ROW SLABS of those volumes (grouped
 * send/recv over RCCL -- mgm_amd/dist.py; an all-reduce would change the fp32 summation order)
 * and every rank finishes its rows with mgm_wta_rows_dev, whose `lr_slabs` is a device buffer
 * [NDIR][nrows][nx][L] holding ALL passes of rows row0..row0+nrows-1 in pass order;
 * out_rows / outcost_rows are device buffers of nrows*nx floats. */
int mgm_aggregate_passes_dev(mgm_ctx *ctx, const mgm_cv *C, const mgm_img *w8, float P1, float P2, int MGM, int use_fh,
                             int first_pass, int n_passes);
/* The same with the caller placing the Lr volumes: pass first_pass+k lands in workspace slot slot0+k of n_slots, and
 * the hand-off region is laid out once for the passes [0, NDIR_total).  For callers that launch the passes of a
 * volume ONE AT A TIME so that pass k's slabs travel while pass k+1 runs (mgm_multi_aggregate, mgm_amd/dist.py). */
int mgm_aggregate_passes_at_dev(mgm_ctx *ctx, const mgm_cv *C, const mgm_img *w8, float P1, float P2, int MGM, int use_fh,
                                int first_pass, int n_passes, int slot0, int n_slots, int NDIR_total);
void *mgm_lr_device_ptr(mgm_ctx *ctx, int slot);
int mgm_wta_rows_dev(mgm_ctx *ctx, const mgm_cv *C, int row0, int nrows, const void *lr_slabs, int NDIR,
                     int fix_overcount, const char *refine, void *out_rows, void *outcost_rows);

/* ---- the same, driven from ONE host thread for n GPUs of a node: mgm_multi ---------------------------------------
 * An mgm_ctx per device plus a transport for the row slabs.  The CPU analogue in the reference is
 * mgm_naive_parallelism (mgm_core.cc:632-831, WITH_MGM2=1): passes in parallel on private Lr volumes, then accumulated
 * -- here always in pass order, so the result is mgm()'s bit for bit.
 *   mgm_multi_create     device_ids: n distinct HIP devices (gfx950).  Transport (mgm_multi_transport tells which):
 *                          "rccl"      grouped ncclSend/ncclRecv on a communicator over the devices (librccl is loaded on
 *                                      first use) -- the default;
 *                          "peer"      the receiving device PULLS each slab with a device-to-device copy on a second
 *                                      stream, ordered by events: MGM_MULTI_TRANSPORT=peer, and what the handle falls back
 *                                      to when librccl cannot be loaded or its communicator cannot be made;
 *                          "loopback"  a device id appears several times (allowed only with MGM_MULTI_LOOPBACK=1): the
 *                                      ranks are contexts on one GPU, copies as for "peer" -- the n-rank path on a one-GPU
 *                                      box (tests).
 *                        On failure *m is NULL and mgm_multi_last_error(NULL) holds the reason.
 *   mgm_multi_ctx        rank k's context: build C[k] on it (mgm_costvolume_build_dev from images uploaded there).
 *   mgm_multi_aggregate  mgm() of ONE volume: C[k] = the same cost volume on every device (rebuilt there from the
 *                        images: cheaper than moving it; MGM_ERR_INVALID if C[k] or w8[k] does not live on device k, or
 *                        out0 / outcost0 not on device_ids[0]), w8 NULL or one weight image per device; rank k runs the
 *                        passes of mgm_multi_plan's block k, the row slabs move (one peer per xGMI link, all links at
 *                        once), every rank sums its rows in pass order and searches them, and the rows are gathered into
 *                        out0 / outcost0.  Synchronous; an exchange that does not complete within
 *                        MGM_MULTI_TIMEOUT_S (default 120) seconds returns MGM_ERR_HIP after aborting the transport (the
 *                        handle is then only good for mgm_multi_destroy).  A rank's failure is reported after EVERY
 *                        rank's queued work has drained, never in the middle of a transfer group.
 *                        MGM_MULTI_OVERLAP=1: ranks with several passes launch them one per launch and each pass's
 *                        slabs leave behind it, while the next pass runs.
 *   mgm_multi_plan       the partition as data: contiguous blocks of passes and of rows per rank (sizes differ by <= 1). */
typedef struct mgm_multi mgm_multi;
int mgm_multi_create(const int *device_ids, int n, mgm_multi **m);
int mgm_multi_destroy(mgm_multi *m);
int mgm_multi_size(const mgm_multi *m);
mgm_ctx *mgm_multi_ctx(mgm_multi *m, int rank);
const char *mgm_multi_last_error(const mgm_multi *m); /* m == NULL: why the last mgm_multi_create of this thread failed */
const char *mgm_multi_transport(const mgm_multi *m);  /* "rccl", "peer" or "loopback" */
int mgm_multi_plan(int n, int NDIR, int ny, int *first_pass, int *n_passes, int *row0, int *nrows);
int mgm_multi_aggregate(mgm_multi *m, const mgm_cv *const *C, const mgm_img *const *w8, float P1, float P2, int NDIR, int MGM,
                        int use_fh, int fix_overcount, const char *refine, mgm_img *out0, mgm_img *outcost0);

/* Test/diagnostic aid: copy pass `pass`'s Lr volume of the LAST mgm_aggregate
 * call on this ctx into `dense` ([ny][nx][L]). */
int mgm_debug_download_lr(mgm_ctx *ctx, int pass, float *dense);

/* Test aid (tests/test_gpu_wta_rel_crafted.py): the device pointer of pass `pass`'s Lr volume of volume 0 of the LAST aggregation on
 * this ctx, when that aggregation ran on the volume's range-proportional copy: [ny * nx][*slots] floats, slot k of a pixel = the
 * disparity record[0] + k, where the pixel's record is the four ints (disparity of slot 0 = its lowest disparity - 1, lowest,
 * highest, 0) at *records + 4 * pixel (device memory too).  *slots is 64 or 128, *cb the bytes per cost code of the copy (1, 2, 4),
 * *pass_stride the floats from one pass's volume to the next; each of the four may be NULL.  NULL where mgm_debug_download_lr
 * refuses its range-proportional form: no such aggregation was the last one, the volume has been refilled since, `pass` out of
 * range.  What is written there is what mgm_wta_windowed_dev and mgm_debug_wta_rel_again_dev search next. */
void *mgm_debug_rel_lr_device_ptr(mgm_ctx *ctx, int pass, int *slots, int *cb, long long *pass_stride, void **records);

/* Test aid (tests/test_gpu_wta_runnerup_crafted.py): the device pointer of pass `pass`'s Lr volume of volume `volume` of the LAST
 * aggregation on this ctx, when that one was a dense run: [ny * nx][*Lk] floats, of which the first L of a pixel are its labels and
 * the slots L..*Lk-1 padding of the launch (*Lk == L: none).  *pass_stride: the floats from one pass's volume to the next; either
 * may be NULL.  Unlike mgm_lr_device_ptr it serves a padded label stride and every volume of a batch.  NULL when the last
 * aggregation was no dense run (none yet, trimmed, range-proportional) or `volume` / `pass` lie outside it.  Launches nothing and
 * changes no record; what is written there is what mgm_wta_windowed_dev, mgm_wta_right_dev and mgm_wta_runnerup_dev search next. */
void *mgm_debug_lr_device_ptr(mgm_ctx *ctx, int volume, int pass, int *Lk, long long *pass_stride);

/* Test aid: the winner search that ended the LAST aggregation of C on this ctx, again -- for an aggregation that ran on C's
 * range-proportional copy: every pixel's window is its own range, the Lr volumes are read as they lie in the workspace, no pass
 * kernel runs.  fix_overcount and refine are this call's (any refinement name); S: NULL, or receives the corrected aggregated
 * volume on the dense hull as mgm_aggregate_dev hands it out there (the caller frees it).  MGM_ERR_INVALID when C was not part
 * of the context's last aggregation, when that one did not run on the range-proportional copy, or with another NDIR than its
 * (mgm_wta_windowed_dev's guard).  No synchronisation. */
int mgm_debug_wta_rel_again_dev(mgm_ctx *ctx, const mgm_cv *C, int NDIR, int fix_overcount, const char *refine, mgm_img *out,
                                mgm_img *outcost, mgm_cv **S);

/* Test/diagnostic aid: the chunk minima (one float per pixel and chunk of 32 labels: [ny][nx][L/32]) that the pass kernel
 * left beside pass `pass`'s Lr volume of volume `slot` of the LAST aggregation call on this ctx, read where the pruned winner
 * search reads them.  MGM_ERR_INVALID when that launch wrote no minima (any launch the pruned search does not follow), when
 * the volume has been refilled since, or when `slot` / `pass` is out of range. */
int mgm_debug_download_lmin(mgm_ctx *ctx, int slot, int pass, float *out);

/* Test/diagnostic aid: what the pruned winner searches of the context's LAST aggregation call did -- pixels searched and
 * chunks of 32 labels whose Lr values were loaded (a plain search loads L/32 per pixel), summed over the call's volumes.
 * Counted only while timing (mgm_timing_enable) or MGM_HIP_DEBUG_STATS is on; both 0 when no search of that call was a
 * pruned one (fall-back cases, MGM_HIP_WTA_PRUNE=0) or nothing was counted. */
int mgm_debug_wta_stats(mgm_ctx *ctx, unsigned long long *pixels, unsigned long long *chunks);

/* Test/diagnostic aid: the pass kernel instance the context's LAST aggregation launched, as a kernel trace spells it --
 * "k_pass2<4, true, false, 2, 1, 1, true, true, true, false>", "k_pass<16, false, true, 4>",
 * "k_pass_rel<true, false, 3, 4, 1, false>", or "k_pass_exact" -- written into buf[cap] (truncated to fit, always terminated).
 * MGM_ERR_INVALID before the context's first aggregation and after mgm_ctx_trim. */
int mgm_debug_last_pass_kernel(mgm_ctx *ctx, char *buf, int cap);

/* Diagnostic (tools/bimodal_probe.py): the rate, in GB/s, at which the store pattern of the pass kernels -- `nstreams`
 * volumes at the stride of the context's last aggregation, written side by side -- lands on the Lr workspace where the
 * allocator placed it.  MGM_ERR_INVALID before the context's first aggregation. */
int mgm_debug_probe_workspace(mgm_ctx *ctx, int nstreams, float *gbps);

/* Device self-test: compares the kernels' three-operation exact x/3 against IEEE
 * division for all 2^32 float32 inputs; *nbad receives the number of inputs
 * whose results differ (NaN == NaN). */
int mgm_selftest_div3(mgm_ctx *ctx, unsigned long long *nbad);

/* ---- sub-pixel refinement: subpixel_refinement_sgm ---------------------- */
/* method in {"none","vfit","parabola","cubic","parabolaOCV"}; unknown => none
 * (mgm_refine.h:28-35).  out/outcost are read and updated.  (vfit is also fused into mgm_aggregate*'s
 * WTA kernel; the other methods run as a second kernel on the corrected S, in mgm_aggregate* too.) */
int mgm_refine_dev(mgm_ctx *ctx, const mgm_cv *S, const char *method, mgm_img *out, mgm_img *outcost);
int mgm_refine(mgm_ctx *ctx, const mgm_cv *S, const char *method, float *out, float *outcost);

/* ---- TSGM_ITER > 1: main()'s loop mgm.cc:377-388 ------------------------------------------------------------
 * The reference builds the cost volume once and calls mgm() TSGM_ITER times with range images that
 * update_dmin_dmax narrows around the previous solution.  The volume is the same every time, hence so are the
 * scan-line passes: only the winner search and the refinement see the new ranges.  mgm_wta_windowed_dev does
 * exactly that part again on the Lr volumes the context still holds from its last mgm_aggregate_dev(C, NDIR)
 * call: the winner of pixel p is the first strict minimum of S over the disparities [(int)dminI(p), (int)dmaxI(p)]
 * (mgm_core.cc:592-609 with S allocated from those images, 426), the refinement gate (mgm_refine.h:58) uses the
 * same window, and a disparity of the window outside C's range holds what it holds there: 0 - (NDIR-1)*INF, or 0
 * without the over-count fix.  Any refinement name. */
int mgm_wta_windowed_dev(mgm_ctx *ctx, const mgm_cv *C, int NDIR, int fix_overcount, const char *refine,
                         const mgm_img *dminI, const mgm_img *dmaxI, mgm_img *out, mgm_img *outcost);
/* The right view's disparity map read out of the LEFT run: searches, for every pixel of a vnx-wide right image, the
 * diagonal of the corrected aggregated volume of the context's last aggregation of C (DESIGN.md "right from left").
 * Right pixel xr with disparity e = -dmax..-dmin names the match of left pixel xr + e with disparity -e; a match
 * outside the left image is +INF.  The winner is the first strict minimum among the finite entries by rising e
 * (mgm_core.cc:592-609 on that diagonal); refine is "none"/NULL or "vfit" (the gate of mgm_refine.h:58 in the right
 * index), the other methods return MGM_ERR_UNSUPPORTED.  outR / outcostR are vnx x ny x 1 images: vnx is taken from
 * them, ny must be C's.  C must be a dense volume (not built from range images: MGM_ERR_UNSUPPORTED) of the context's
 * last aggregation with NDIR passes, in any slot of a batch (else MGM_ERR_INVALID).  No synchronisation. */
int mgm_wta_right_dev(mgm_ctx *ctx, const mgm_cv *C, int NDIR, int fix_overcount, const char *refine,
                      mgm_img *outR, mgm_img *outcostR);
/* The runner-up search (DESIGN.md "runner-up, confidence, uniqueness"; this library's own mode, the reference has none): a third
 * search of the corrected aggregated volume S of the context's last aggregation of C.  Per pixel, with o = d - dmin:
 *   winner     o1 = the first strict minimum among the finite entries of S by rising o (mgm_core.cc:592-609: what mgm_aggregate*
 *              returns without refinement); out1 = (float)(o1 + dmin), cost1 = S(o1) -- always the unrefined S, never vfit's
 *              v_min; no finite entry: out1 = NaN, cost1 = +INF
 *   runner-up  o2 = the first strict minimum among the finite entries with |o - o1| > radius; out2 = (float)(o2 + dmin),
 *              cost2 = S(o2); no winner or no such entry: out2 = NaN, cost2 = +INF
 * radius >= 0 (negative: MGM_ERR_INVALID); a radius at or beyond the label count is valid and leaves no runner-up anywhere.
 * out2 / cost2 (and out1 / cost1, each of which may be NULL) are nx x ny x 1 images of C's size (else MGM_ERR_INVALID).  C must
 * be a dense volume (built from range images: MGM_ERR_UNSUPPORTED; its last aggregation ran on the range-proportional copy:
 * MGM_ERR_UNSUPPORTED) of the context's last aggregation with NDIR passes, in any slot of a batch (else MGM_ERR_INVALID).  The
 * call leaves what the context holds of that aggregation untouched: mgm_wta_windowed_dev / mgm_wta_right_dev give the same maps
 * before and after it.  No synchronisation. */
int mgm_wta_runnerup_dev(mgm_ctx *ctx, const mgm_cv *C, int NDIR, int fix_overcount, int radius,
                         mgm_img *out2, mgm_img *cost2, mgm_img *out1, mgm_img *cost1);
/* Confidence and uniqueness filter from the two costs of mgm_wta_runnerup_dev, per pixel in float:
 *   conf = 1.0f - cost1 / cost2      one division, one subtraction, whatever IEEE gives: no runner-up -> 1, no winner
 *                                    (INF / INF) -> NaN, 0 / 0 -> NaN
 *   out  = conf < ratio ? NaN : d    (a NaN conf keeps d)
 * d is any map of that size (the command line passes the refined one).  out and conf may each be NULL, not both; out may be d.
 * All images are one-channel and of one size, ratio is finite and in [0, 1] (else MGM_ERR_INVALID).  No synchronisation. */
int mgm_uniqueness_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *cost1, const mgm_img *cost2, float ratio,
                       mgm_img *out, mgm_img *conf);
/* The consensus votes (DESIGN.md "consensus votes"; this library's own measure, the reference has none): how many of the NDIR
 * scan-line passes of the context's last aggregation of C, each taken ALONE, pick the label the map d holds.  Per pixel x:
 *   pass winner  w_p = the first strict minimum, by rising label, among the finite entries of Lr_p(x, .) over the labels the pixel
 *                owns: 0..L-1 of a dense volume, its own range [(int)lo, (int)hi] inside the volume for a ragged one.  Padding slots
 *                of a padded label stride and slots outside the pixel's range are never candidates, whatever they hold; equal values,
 *                -0 / +0 included, go to the smaller label; no finite entry: the pass has no winner
 *   vote         w_p exists and fabsf((float)(w_p + dmin) - d(x)) <= tol: one float subtraction, a NaN or infinite d(x) gets no vote
 *   votes(x)     = (float) number of voting passes, 0..NDIR
 *   winners      nx x ny x NDIR, planar: winners[p](x) = (float)(w_p + dmin), NaN without a winner
 * No cost is read and no sum is formed, so the definition is one for a dense volume, a ragged volume whose aggregation ran on its
 * dense hull and one whose aggregation ran on the range-proportional copy: the call is never MGM_ERR_UNSUPPORTED for a ragged volume,
 * and the two ragged routes agree bit for bit.  d is any nx x ny x 1 map in labels (a refined, windowed or sub-pixel map is fine).
 * votes and winners may each be NULL, not both; d may be NULL when only winners is asked for.  MGM_ERR_INVALID: a null argument, a
 * size or channel mismatch, votes or winners aliasing d (or each other), tol negative or not finite, NDIR outside 1..8, a volume that
 * is not part of the context's last aggregation with NDIR passes (a trimmed context, a volume or a range-proportional copy refilled
 * since, an earlier chunk of a chunked batch).  The call leaves what the context holds of that aggregation untouched.  No
 * synchronisation; the timing table lists the call as k_wta_consensus, with the family that ran (k_wta_consensus_stream / _any /
 * _rel) as a second name.  MGM_HIP_WTA_CONSENSUS_ANY=1 sends every call to the generic kernel, MGM_HIP_WTA_CONSENSUS_WG=<workgroups
 * per CU> lowers the grid's cap (both for tests, read at every call). */
int mgm_wta_consensus_dev(mgm_ctx *ctx, const mgm_cv *C, int NDIR, const mgm_img *d, float tol, mgm_img *votes, mgm_img *winners);
/* The consensus filter, per pixel: out = votes < (float)minvotes ? NaN : d.  minvotes >= 0 (0 keeps every pixel); out may be d, not
 * votes; all images one-channel and of one size (else MGM_ERR_INVALID).  No synchronisation.
 * The command line: -C FILE writes the left run's votes, MGM_CONSENSUS=k (0: off) filters each run's map, MGM_CONSENSUS_TOL (1) is
 * the tolerance; `mgm --help` does not name them yet (its text is pinned by a recorded table). */
int mgm_consensus_filter_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *votes, int minvotes, mgm_img *out);
/* The speckle filter (DESIGN.md "speckle filter"; this library's own step, the reference has none): small islands of disparity go.
 * d is an nx x ny x 1 map, maxsize >= 0, maxdiff >= 0 (+INF allowed; negative or NaN: MGM_ERR_INVALID as maxsize < 0 is).
 *   valid pixel  d(p) is finite; NaN and +-INF pixels belong to no component and are copied to out bit for bit
 *   edge         two 4-neighbours p, q, both valid, are joined iff fabsf(d(p) - d(q)) <= maxdiff: one float subtraction, so -0 and
 *                +0 are joined and a difference that overflows to +INF is joined under maxdiff = +INF only
 *   component    a connected component of that graph (chained: a ramp 0, 1, 2, ..., N is ONE component under maxdiff = 1);
 *                size(p) = the number of pixels of p's component
 *   out(p)       = valid(p) && size(p) <= maxsize ? NaN : d(p)   (OpenCV's filterSpeckles: a region of exactly maxsize pixels goes;
 *                maxsize = 0 leaves out == d bit for bit)
 *   size_map(p)  = (float)size(p) on valid pixels, 0 on the others
 * 4-connectivity, one channel.  out and size_map may each be NULL, not both; out may be d, size_map must be an image of its own; all
 * images are one-channel and of one size (else MGM_ERR_INVALID).  More than 2^31 - 1 pixels: MGM_ERR_UNSUPPORTED.  The result
 * depends on no traversal order and the filter is idempotent.  Scratch: two int32 planes of the map's size, kept by the context
 * (mgm_ctx_trim releases them).  No synchronisation; the timing table lists the call as k_speckle. */
int mgm_speckle_dev(mgm_ctx *ctx, const mgm_img *d, int maxsize, float maxdiff, mgm_img *out, mgm_img *size_map);
/* Hole filling (DESIGN.md "hole filling"; this library's own step, the reference has none): every rejected pixel takes a value from
 * its nearest valid neighbours along 2, 4 or 8 rays.  d is an nx x ny x 1 map, mode "median", "min" or "max", dirs 2, 4 or 8,
 * maxdist >= 0 (0: no limit).
 *   valid pixel  d(p) is finite; NaN and +-INF pixels are holes
 *   directions   0 (+1,0)  1 (-1,0)  2 (0,+1)  3 (0,-1)  4 (+1,+1)  5 (-1,+1)  6 (+1,-1)  7 (-1,-1); dirs takes the first 2, 4 or 8
 *   candidate    c_k(p) = d(p + t * step_k) for the smallest t >= 1 at which that pixel lies inside the image and is valid; none when
 *                the ray leaves the image first, or when maxdist > 0 and t > maxdist.  Rays read the ORIGINAL map only and pass
 *                over other holes
 *   fill value   of a hole with n >= 1 candidates: order them by value, ascending, with the IEEE comparison, equal values by
 *                direction index (a stable sort of the candidates in direction order: it decides which of -0 and +0 is written);
 *                min = v[0], max = v[n-1], median = v[n/2] (the upper median).  No float arithmetic: always one of d's values
 *   out(p)       = d(p) bit for bit on valid pixels and on holes without a candidate (NaN payloads and +-INF stay), else the fill value
 *   filled(p)    = 1.0f where a hole received a value, 0.0f elsewhere
 * One channel; one rule for every hole (occlusions and mismatches apart: mgm_classify_holes_dev and the classified fill below).  out and filled may
 * each be NULL, not both; out may be d, filled must be an image of its own; all images are one-channel and of one size; a mode
 * that is NULL or none of the three names, dirs outside {2, 4, 8}, maxdist < 0: MGM_ERR_INVALID.  More than 2^31 - 1 pixels:
 * MGM_ERR_UNSUPPORTED.  The result depends on no traversal order; the step is NOT idempotent (a second application may fill what the
 * first could not reach).  Scratch: dirs float planes of the map's size and the bands' carries, kept by the context (mgm_ctx_trim
 * releases them).  No synchronisation; the timing table lists the call as k_holes. */
int mgm_fill_holes_dev(mgm_ctx *ctx, const mgm_img *d, const char *mode, int dirs, int maxdist, mgm_img *out, mgm_img *filled);
/* Hole classification (DESIGN.md "hole classification"; this library's own step, the reference has none; after Hirschmueller 2008,
 * section 2.6): every hole of d is an occlusion or a mismatch, decided from the other view.  d is the nx x ny x 1 map with holes,
 * other the OTHER view's vnx x ny x 1 map as it went INTO the left-right test (not the checked one: a checked map can never
 * point back at a pixel that test rejected), dmin <= dmax the disparity range, tau finite and >= 0, cls an nx x ny x 1 image.
 *   cls(x,y) = 0.0f  where d(x,y) is finite
 *   cls(x,y) = 2.0f  (mismatch) at a hole iff an integer xr exists with max(0, x+dmin) <= xr <= min(vnx-1, x+dmax), other(xr,y)
 *                    finite and fabsf(((float)xr + other(xr,y)) - (float)x) <= tau: some pixel of the other view lands on it.  In
 *                    float, in that order, no contraction, one comparison; a landing coordinate that overflows to +-INF never matches
 *   cls(x,y) = 1.0f  (occlusion) at every other hole, those whose whole range falls outside `other` included
 * The convention is mgm_leftright_dev's: left x with disparity d names right x + d.  A NULL argument, an image that is not
 * one-channel, other->ny != d->ny, cls not of d's size or cls == d or cls == other, dmin > dmax, tau negative or not finite:
 * MGM_ERR_INVALID.  More than 2^31 - 1 pixels: MGM_ERR_UNSUPPORTED.  Any range length: the work per hole grows with it, the memory
 * does not.  No scratch.  No synchronisation; the timing table lists the call as k_holes_classify. */
int mgm_classify_holes_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *other, int dmin, int dmax, float tau, mgm_img *cls);
/* The classified fill: mgm_fill_holes_dev with one rule for the occlusions and one for the mismatches.  Candidates, directions, dirs,
 * maxdist, the ordering by (value, direction index), out on valid pixels and on holes without a candidate, and filled are exactly
 * mgm_fill_holes_dev's.  Mode names: "median", "min", "max" and
 *   seclow  = v[min(1, n-1)]    the second lowest candidate (the lowest when there is one)
 *   sechigh = v[max(n-2, 0)]    the second highest
 * A hole with cls(p) == 1.0f takes mode_occ, every other hole mode_mis, whatever else cls holds there (NaN included); cls is read at
 * holes only.  An occlusion wants the BACKGROUND's second candidate: which of the two that is depends on the sign of the caller's
 * disparities -- with a range like -r -64 -R 0 the background is the higher value, sechigh.  No float arithmetic: always one of d's
 * values.  out and filled may each be NULL, not both; out may be d; filled must be an image of its own (not d, cls or out); all
 * images one-channel and of d's size; a NULL argument, a mode name outside the five, dirs outside {2, 4, 8}, maxdist < 0:
 * MGM_ERR_INVALID.  More than 2^31 - 1 pixels: MGM_ERR_UNSUPPORTED.  mode_occ == mode_mis (one of the three old names) is
 * mgm_fill_holes_dev bit for bit.  Scratch: mgm_fill_holes_dev's, shared with it.  No synchronisation; the timing table lists the
 * call as k_holes.  The class map is the caller's image: the command line has no file option for it. */
int mgm_fill_holes_classified_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *cls, const char *mode_occ, const char *mode_mis,
                                  int dirs, int maxdist, mgm_img *out, mgm_img *filled);
/* Solution energy (DESIGN.md "solution energy"): what a disparity map d costs in the terms of the functional that the aggregation
 * minimises -- the reference's three figures (evaluate_energy_4connected, mgm_print_energy.h:17-96; what TSGM_DEBUG=1 prints) and this
 * library's own model energy.  C is the cost volume of the run (for a sub-pixel fine volume d is in fine labels too), d any
 * nx x ny x 1 map.  All per-pixel arithmetic is fp32, one rounding per operation, nothing contracted.
 *   C(p, l)      the cost of label l at pixel p; +INF for a label the pixel does not own: outside [dmin, dmax], outside the pixel's
 *                own range of a ragged volume, and for a d(p) that is not finite or has |d(p)| >= 2^24
 *   kinds 0-2    o = d(p); G = 0 + C(p, (int)o) (truncation); then for t = 0..3 with r = p + dir[t], q = p + dir[t+1], dirs (-1,0) (0,1)
 *                (1,0) (0,-1) (-1,0), skipped unless BOTH r and q lie inside the image (so a one-pixel-wide or one-row map has no
 *                edge term at all):
 *                  kind 0 (truncated L1)  G += (fabsf(d(r) - o) <= 1 ? P1 : P2) / 4
 *                  kind 1 (L1)            G += fabsf(d(r) - o) / 4
 *                  kind 2 (L2)            G += sqrtf((d(r) - o)^2 + (d(q) - o)^2) / 4      (correctly rounded)
 *                E(p) = G.  Whatever IEEE gives: a NaN neighbour makes kinds 1 and 2 NaN and takes the P2 branch of kind 0.  (The
 *                reference's file /tmp/ENERGY_L1trunc.tif holds the L1 map under that name; here E of kind 0 is the truncated map.)
 *   kind 3       the model energy over the first `connectivity` (4 or 8) neighbours in the order of the weight planes, W E S N NW NE
 *                SE SW.  d(p) not finite: E(p) = NaN.  Else data = C(p, (int)rintf(d(p))); for each k whose neighbour q lies inside
 *                the image and has a finite d(q): a = fabsf(d(q) - d(p)), w = w8[k](p) (1 without w8),
 *                  use_fh = 0 (Hirschmueller)      V = a == 0 ? 0 : a <= 1 ? fminf(P1*w, P2*w) : P2*w
 *                  use_fh = 1 (truncated linear)   V = fminf((P1*w) * a, P2*w)
 *                smooth = 0.5f * (((0 + V_k0) + V_k1) + ...) in k order, E(p) = data + smooth.  Every undirected edge is counted from
 *                both ends at half weight: the total is sum data + sum over edges of mean(w_pq, w_qp) * V, whatever the weights are.
 *                It is the energy of the pairwise functional, NOT of MGM's message sums: MGM minimises it approximately.
 *   totals       serial: the fp32 sum of E in raster order, 0 + E(0) + E(1) + ... -- the number the reference prints, formed on the
 *                host from the map the device wrote.  total, data, smooth: fp64 sums of E, of the data terms and of the edge terms
 *                (kinds 0-2: 0 + t_0 + t_1 ... in fp32 per pixel; kind 3: smooth) over the pixels with a finite d(p), which `finite`
 *                counts; `pixels` = nx * ny.  One fp64 partial per block of 256 pixels in raster order, added in index order: no float
 *                atomics, two calls give the same bits.
 * The volume is read in whatever copy is current (fp32, one- or two-byte codes, the padded compact copy, the range-proportional
 * copy of a ragged volume that has no other): one cost per pixel, nothing is decoded, made or checked.  E and t may each be NULL,
 * not both.  With t the call synchronises; without it it does not.  It leaves what the context holds of its last aggregation
 * untouched.  MGM_ERR_INVALID: a null argument, kind outside 0..3, P1 negative or not finite, P2 negative or NaN (+INF is valid),
 * kind 3 with a connectivity other than 4 or 8, d or E not nx x ny x 1 of the volume's size, E == d, w8 not nx x ny x 8, a volume
 * whose refill failed.  More than 2^31 - 1 pixels: MGM_ERR_UNSUPPORTED.  The timing table lists the call as k_energy.
 * The command line: TSGM_DEBUG=1 prints the reference's debug lines, the three figures of every iteration and run among them;
 * MGM_ENERGY=4|8 prints the model energy of each run and iteration on stderr, MGM_ENERGY_MAP=FILE writes the left run's last map of it. */
typedef struct mgm_energy_params {
    int kind;            /* 0 L1trunc, 1 L1, 2 L2: evaluate_energy_4connected; 3: the model energy */
    float P1, P2;        /* as given (the caller has multiplied by the channel count) */
    int connectivity;    /* kind 3: 4 or 8 */
    int use_fh;          /* kind 3: 0 Hirschmueller, 1 truncated linear */
    const mgm_img *w8;   /* kind 3: NULL (ones) or the 8-channel weight image of mgm_weights_dev / a caller's own */
} mgm_energy_params;
typedef struct mgm_energy_totals {
    float serial;        /* fp32 sum of the map in raster order: what the reference returns */
    double total, data, smooth;       /* fp64 sums over the pixels counted in `finite` */
    unsigned long long finite, pixels;
} mgm_energy_totals;
int mgm_energy_dev(mgm_ctx *ctx, const mgm_cv *C, const mgm_img *d, const mgm_energy_params *p, mgm_img *E, mgm_energy_totals *t);
/* update_dmin_dmax (mgm.cc:120-158; main() uses slack 3, radius 2) followed by the two
 * remove_nonfinite_values_Img calls (mgm.cc:387-388): dminI/dmaxI are updated in place from the disparity map. */
int mgm_update_ranges_dev(mgm_ctx *ctx, const mgm_img *outoff, mgm_img *dminI, mgm_img *dmaxI, int slack, int radius);

/* ---- what main() does to the disparity maps right after the path (device images in, device images out) ---- */
/* median_filter (img_tools.h:203-238, called at mgm.cc:396, 419 when MEDIAN != 0): per channel, the window
 * (2*radius+1)^2 clipped at the border, NaN samples ignored, the upper median v[n/2]; an all-NaN window
 * leaves the pixel unchanged.  Any radius >= 1 (beyond 7 the order statistic is found by radix selection instead of
 * pairwise counting: 33 sweeps of the window per pixel, so the call is bounded -- MGM_ERR_UNSUPPORTED when
 * 33 * (2*radius+1)^2 * nx*ny*nch exceeds 1e13 window reads, i.e. beyond radius ~190 at 1920x1080; up to that it
 * takes at most about a minute).  out must have in's size (and must not be in). */
int mgm_median_dev(mgm_ctx *ctx, const mgm_img *in, int radius, mgm_img *out);
/* leftright_test (mgm.cc:68-91, called at 420-423): out[x,y] = d[x,y] if Lx = round(x + d) lies inside `other`
 * and |Lx + other[Lx,y] - x| <= tau, NaN otherwise.  d and out have one size, `other` may have another width. */
int mgm_leftright_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *other, float tau, mgm_img *out);
/* the back-projected image main() writes as its optional third output (mgm.cc:433-443): v sampled at x + disp
 * (integer truncation of the reference's float index), u where that falls outside v. */
int mgm_backproject_dev(mgm_ctx *ctx, const mgm_img *u, const mgm_img *v, const mgm_img *disp, mgm_img *out);

/* ---- coarse-to-fine (multiscale) driver ------------------------------------------------------------------------
 * The reference has no multiscale program; it ships the one step that only makes sense in one: update_dmin_dmax
 * (mgm.cc:120-158) gives a pixel whose disparity is NaN -- one the left-right test rejected -- the GLOBAL range.  The
 * definition below is this project's own, made of reference steps and three resampling rules that are exact in fp32
 * (DESIGN.md "multiscale" has it in full).  Levels s = 0 (full size) .. S-1; n_{s+1} = (n_s + 1) / 2 for each of nx, ny,
 * vnx, vny.
 *   image zoom-out   out(x,y) = ((a + b) + (c + d)) * 0.25f over the 2x2 block at (2x,2y), indices clamped to the image
 *   range zoom-out   lo' = floorf(0.5f * min lo), hi' = ceilf(0.5f * max hi) over the same four pixels
 *   prior -> ranges  U(x,y) = 2.0f * D(x >> 1, y >> 1) of the coarser level's FINAL map (NaNs included), then
 *                    update_dmin_dmax(U, lo, hi, slack, radius) + the two remove_nonfinite_values_Img calls on the level's
 *                    base ranges; no clipping afterwards.
 * mgm_multiscale_levels: the effective level count -- the largest S <= nscales (1..8) whose coarsest level still has
 * min(nx, ny, vnx, vny) >= 16, at least 1 -- and, if dims != NULL, its sizes dims[s] = {nx, ny, vnx, vny}.  Pure host
 * arithmetic: needs no device.  Returns S, or -MGM_ERR_INVALID (sizes < 1, nscales outside 1..8). */
int mgm_multiscale_levels(int nx, int ny, int vnx, int vny, int nscales, int *dims);
/* *out NULL: a new ((nx+1)/2, (ny+1)/2, nch) image; else one of that size, refilled.  `in` must hold no NaN for the
 * result to be the definition's (the inputs of the path are NaN-free, mgm.cc:335-336). */
int mgm_zoom_out_dev(mgm_ctx *ctx, const mgm_img *in, mgm_img **out);
int mgm_ranges_zoom_out_dev(mgm_ctx *ctx, const mgm_img *lo, const mgm_img *hi, mgm_img **lo2, mgm_img **hi2);
/* The prior -> ranges step as ONE kernel that reads only the coarse map: coarse_disp is ((nx+1)/2, (ny+1)/2), lo / hi are
 * the fine level's nx*ny base ranges on entry and its updated ranges on return -- bit for bit what zooming the map in
 * and mgm_update_ranges_dev give.  radius 0..16.  hull_min / hull_max (both or neither): min (int)lo / max (int)hi of
 * the result, what mgm_costvolume_build_ranged_dev wants; asking for them synchronises (two words come back). */
int mgm_ranges_from_coarse_dev(mgm_ctx *ctx, const mgm_img *coarse_disp, mgm_img *lo, mgm_img *hi, int slack, int radius,
                               int *hull_min, int *hull_max);

typedef struct mgm_ms_level {  /* what one level of mgm_multiscale_pair_dev ran on; index 0 = left->right, 1 = right->left */
    int nx, ny, vnx, vny;
    int hull_min[2], hull_max[2]; /* min (int)lo / max (int)hi of each run's ranges (a volume batched with the other run's
                                     may have been built on a wider hull: labels nobody owns read +INF) */
    int weighted[2];              /* the run's weights hold a value != 1: mgm() takes the weighted update functions */
    int batched;                  /* both runs shared one launch of the pass kernel */
} mgm_ms_level;

typedef struct mgm_ms_params {
    unsigned struct_size; /* sizeof(mgm_ms_params) of the caller: the struct may grow at its end */
    int nscales;          /* requested levels, 1..8 (fewer run when the images are too small: mgm_multiscale_levels) */
    int slack, radius;    /* of the prior -> ranges step (the reference's defaults: 3, 2) */
    int dmin, dmax;       /* -r / -R */
    const mgm_img *lo, *hi; /* optional level-0 range images of the left->right run (-m / -M after main()'s fix-ups,
                               mgm.cc:342-353): both or neither */
    float P1, P2;         /* already multiplied by the channel count (mgm.cc:356-357) */
    int NDIR, TSGM, use_fh, fix_overcount;
    float aP2, aThresh;   /* aP2 != 1: image-dependent weights, computed per level from that level's images */
    const char *prefilter, *distance;
    float truncDist;
    int census_win;
    const char *refine;
    int iterations;       /* TSGM_ITER as main() counts it (>= 0; 0: mgm() is never called, the maps are zero) */
    int median;           /* MEDIAN radius, 0 = none */
    int testlrrl;         /* TESTLRRL: 0 = the left->right chain only */
    float tau;            /* TESTLRRL_TAU */
    int *levels_run;      /* optional out: the effective level count */
    mgm_ms_level *levels; /* optional out: `nscales` entries, [s] filled for every level that ran */
    mgm_img *outR_nolr;   /* optional out (NULL or absent: nothing happens): vnx*vny, the finest level's right map after MEDIAN and
                             before its left-right test -- what mgm_classify_holes_dev wants as `other`; untouched with testlrrl = 0 */
    /* the consensus votes (mgm_wta_consensus_dev), at the finest level only, on each run's map after its iterations and refinement and
     * before MEDIAN and the left-right test; absent (an older struct_size) or zero: nothing happens */
    float consensus_tol;  /* the tolerance, finite and >= 0 (looked at only when one of the next two asks for the step) */
    int consensus_min;    /* > 0: each run's map becomes NaN where fewer passes vote for it (mgm_consensus_filter_dev); < 0: MGM_ERR_INVALID */
    mgm_img *votesL;      /* optional out: nx*ny, the left->right run's votes (zeros with iterations = 0: no pass has voted) */
} mgm_ms_params;

/* One stereo pair, coarse to fine.  Per level exactly what the `mgm` command line does for a pair (weights, ranged cost
 * volumes, mgm(), refinement, iterations 2..TSGM_ITER, MEDIAN, the two left-right tests) with range images for BOTH
 * runs; every level but the coarsest takes its ranges from the coarser level's final maps.  nscales = 1 (or images too
 * small for a second level) is the single-scale result bit for bit.  The two runs of a level share one launch of the pass
 * kernel when mgm_aggregate_batch_dev takes them and otherwise run one after the other: same results.  Between levels
 * only the two hull integers per run (and one flag per weighted run) come back to the host; no image is downloaded or
 * uploaded.  outL / costL: nx*ny; outR / costR: vnx*vny or NULL (with testlrrl = 0 they are left untouched);
 * outL_nolr: nx*ny or NULL, the left map before the left-right test.  Not on a pipelined context with deferred work of
 * its own outputs; a failure frees every intermediate object and leaves the context usable. */
int mgm_multiscale_pair_dev(mgm_ctx *ctx, const mgm_img *u, const mgm_img *v, const mgm_ms_params *p, mgm_img *outL,
                            mgm_img *costL, mgm_img *outR, mgm_img *costR, mgm_img *outL_nolr);

#ifdef __cplusplus
}
#endif
#endif /* MGM_HIP_H_ */
