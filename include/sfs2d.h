/*
 * sfs2d.h -- C ABI of the MI355X windowed 2D-SFS composite-likelihood scan.
 *
 * Drop-in boundary for the hot path of uricchio/2DSFS-scan: the per-window 2D-SFS + folded
 * 1D-SFS accumulation and the T2D / T1D multinomial log-likelihood ratios against a
 * background SFS (scripts/src/twoDSFS_class.py, scripts/sims_scan.py).  The reference has no
 * FFI layer -- its boundary is the Python class `LikelihoodInference_jointSFS`
 * (twoDSFS_class.py:20-33) -- so these entry points are what that class's methods bind through
 * ctypes:
 *
 *   sfs2d_data_upload / _wrap_device  <- the SNP dict built by make_data_dict_vcf (36-138),
 *                                        packed into SoA (sorted as in combined_scan 828-835)
 *   sfs2d_bg_hist                     <- calculate_2d_sfs (140-232) + calculate_1d_sfs (398-444)
 *                                        over a whole chromosome / data set (background SFS)
 *   sfs2d_plan_create + sfs2d_plan_run <- the window loop of combined_scan (787-991),
 *                                        scan_chooseChr (993), scan_precomputed_BG (1161),
 *                                        scan_*_bySNPs (1303, 1422), sims_scan.process_window (451):
 *                                        per window calculate_2d_sfs + fold_1d_sfs(calculate_1d_sfs)
 *                                        + calculate_likelihood_2D (625-684) / _1D (478-537)
 *   sfs2d_scan                        <- one-shot plan_create + plan_run + copy-out
 *
 * Conventions: every call returns 0 on success or a negative SFS2D_E* code; the message is
 * available from sfs2d_last_error(ctx).  Nothing throws or aborts across the ABI.  The caller
 * owns every host buffer; the library owns the device buffers inside ctx / data / plan.
 * One ctx per GPU; calls on one ctx must be serialised by the caller.  All work is enqueued on
 * the ctx's HIP stream (sfs2d_ctx_set_stream to share a stream with another runtime).
 */
#ifndef SFS2D_H
#define SFS2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5-6): sfs2d_ctx_set_stream(ctx, NULL) selects the HIP null stream (1: the ctx's own),
 * sfs2d_ctx_use_own_stream / sfs2d_ctx_get_stream added, the sfs2d_dist_* entry points removed;
 * sfs2d_graph_* added (round 6, additive); sfs2d_plan_create_sliding / sfs2d_plan_attach_sliding added
 * (additive: sfs2d_params keeps its layout, the step is an argument); sfs2d_plan_null_run / _null_read added
 * (additive); sfs2d_plan_null_run_blocks added (additive: sfs2d_null_params keeps its layout, the block length is
 * an argument); sfs2d_plan_diversity / _diversity_read and sfs2d_diversity added (additive);
 * sfs2d_plan_create_regions / sfs2d_plan_attach_regions added (additive: the intervals are arguments);
 * sfs2d_plan_spectra / _spectra_read added (additive); sfs2d_plan_project / _project_read and
 * sfs2d_project_weights added (additive); sfs2d_plan_project_scan / _project_scan_read added (additive);
 * sfs2d_plan_project_null / _project_null_read added (additive) */
#define SFS2D_ABI_VERSION 2

/* status codes */
#define SFS2D_OK 0
#define SFS2D_E_ARG (-1)       /* invalid argument (sizes, modes, null pointers) */
#define SFS2D_E_HIP (-2)       /* HIP runtime error (message has the HIP string) */
#define SFS2D_E_NOMEM (-3)     /* device allocation failed */
#define SFS2D_E_KEY (-4)       /* an alt count > 2*pop_size: the reference raises KeyError (calculate_1d_sfs:433) */
#define SFS2D_E_GRID (-5)      /* a folded 2D bin lies outside the (2n1+1)x(2n2+1) grid */
#define SFS2D_E_CAP (-6)       /* output capacity too small (*nwin_out holds the needed size) */

/* window modes */
#define SFS2D_WINDOW_BP 0      /* fixed-bp windows, window id (pos-1)//ws per chromosome (twoDSFS_class.py:894, 948) */
#define SFS2D_WINDOW_SNPS 1    /* fixed SNP-count windows, incomplete tail dropped (1515-1535) */

/* background modes */
#define SFS2D_BG_PER_CHROM 0   /* each chromosome's own SNPs form its background (combined_scan 809-825) */
#define SFS2D_BG_SUPPLIED 1    /* one background for all windows (scan_chooseChr / precomputed / sims) */

/* plan flags */
#define SFS2D_F_PREV_EXTRA 1u  /* also evaluate the previous window's 1D SFSs against the LAST window's
                                  chromosome background (combined_scan final block, 951-989, quirk Q9) */

#define SFS2D_F_FST 2u         /* also compute Hudson's Fst per window slot (not in the reference),
                                  read with sfs2d_plan_fst_read / sfs2d_plan_fst_buffer */

/* window record flags */
#define SFS2D_W_EMPTY 0x80000000u  /* slot holds no SNP (fixed-bp slot between SNPs): not a window */
#define SFS2D_W_BG2_ZERO 0x1u      /* background 2D inner sum == 0  -> None / ZeroDivisionError */
#define SFS2D_W_BG1A_ZERO 0x2u
#define SFS2D_W_BG1B_ZERO 0x4u
#define SFS2D_W_EXTRA 0x40000000u  /* record is the Q9 helper (see SFS2D_F_PREV_EXTRA) */

typedef struct sfs2d_ctx sfs2d_ctx;
typedef struct sfs2d_data sfs2d_data;
typedef struct sfs2d_plan sfs2d_plan;
typedef struct sfs2d_graph sfs2d_graph;

typedef struct {
  int32_t n1p, n2p;       /* pop1_size, pop2_size: diploid individuals (twoDSFS_class.py:22); grid (2n1p+1)x(2n2p+1) */
  int32_t fold;           /* joint 2D fold: swap ref/alt in both pops if alt1+alt2 > n1p+n2p (197-206) */
  int32_t window_mode;    /* SFS2D_WINDOW_BP / SFS2D_WINDOW_SNPS */
  int64_t window;         /* window size in bp, or SNPs per window */
  int32_t bg_mode;        /* SFS2D_BG_PER_CHROM / SFS2D_BG_SUPPLIED */
  int32_t ann_want;       /* variant_type filter: annotation id to keep, -1 = no filter (185-187, 291-302) */
  int32_t has_start, has_end; /* SFS position filter start_position / end_position (179-182) */
  int64_t start_pos, end_pos;
  uint32_t flags;         /* SFS2D_F_* */
  uint32_t scan_wgs_per_cu; /* 0: the scan kernel's grid is one resident wave of workgroups (all that fit);
                               k > 0: at most k workgroups per CU -- leaves CUs to the next pass's k_prep
                               when independent passes overlap on several streams (sfs2d_plan_run_streams) */
} sfs2d_params;

/* one record per window slot (64 bytes) */
typedef struct {
  uint32_t chrom;         /* chromosome index in the data set's (sorted) chromosome list */
  uint32_t wid;           /* window index within the chromosome: (pos-1)//ws, or SNP-window ordinal */
  uint32_t begin, end;    /* SNP index range [begin, end) in the data set */
  uint32_t snp_count;     /* count_snps (291-302): SNPs in the window matching variant_type */
  uint32_t n2;            /* 2D foreground total over inner bins bins[1:-1] (N of T2D) */
  uint32_t n2_all;        /* 2D foreground total over all bins (scan_*_bySNPs skip test, 1376/1496) */
  uint32_t n1a, n1b;      /* folded 1D foreground totals over inner bins 1..pop_size-1 */
  uint32_t flags;         /* SFS2D_W_* */
  double t2d, t1d_p1, t1d_p2; /* NaN-boxed "None" is not used: validity = n>0 and !BG*_ZERO */
} sfs2d_window;

/* context */
int sfs2d_ctx_create(int device, sfs2d_ctx** out);
int sfs2d_ctx_destroy(sfs2d_ctx* ctx);
const char* sfs2d_last_error(const sfs2d_ctx* ctx);
/* Stream the ctx enqueues on.  sfs2d_ctx_set_stream(ctx, s): the caller's HIP stream s; NULL is the
 * HIP null stream (the legacy default stream: ordered with every blocking stream of the process, e.g.
 * torch's default stream), never a private one.  sfs2d_ctx_use_own_stream: the ctx's own non-blocking
 * stream (the state after sfs2d_ctx_create), which NOTHING orders against the caller's streams --
 * synchronise before handing buffers across.  The class state these replace is the reference object's
 * (twoDSFS_class.py:21-33): one ctx per GPU, calls serialised by the caller. */
int sfs2d_ctx_set_stream(sfs2d_ctx* ctx, void* hip_stream);
int sfs2d_ctx_use_own_stream(sfs2d_ctx* ctx);
/* the HIP stream the ctx currently enqueues on (NULL = the null stream; after sfs2d_ctx_create or
 * sfs2d_ctx_use_own_stream, the handle of the ctx's own stream) -- e.g. to pass it to
 * sfs2d_plan_run_streams or to order a caller's stream after the ctx's work */
int sfs2d_ctx_get_stream(const sfs2d_ctx* ctx, void** hip_stream);
/* SFS2D_ABI_VERSION of the loaded library (negative: an ablation build for timing experiments, whose
 * results are wrong -- loaders must refuse it) */
int sfs2d_abi_version(void);

/* data set: packed SNPs in scan order (sorted by chromosome string, then position) */
int sfs2d_data_upload(sfs2d_ctx* ctx, const uint32_t* counts, const uint32_t* pos, const uint16_t* ann_id,
                      int64_t n, const int64_t* chrom_off, int32_t nchrom, sfs2d_data** out);
/* wrap caller-owned DEVICE arrays (no copy); chrom_off / chrom_last_pos are HOST arrays */
int sfs2d_data_wrap_device(sfs2d_ctx* ctx, const uint32_t* d_counts, const uint32_t* d_pos,
                           const uint16_t* d_ann_id, int64_t n, const int64_t* chrom_off,
                           const uint32_t* chrom_last_pos, int32_t nchrom, sfs2d_data** out);
/* A data set whose positions the library owns (sfs2d_data_upload, sfs2d_data_synth_sims) also owns a position
 * index, built on the device (0.1 ms for 5e7 SNPs) when the first plan that takes its window slots from it is
 * created (sfs2d_plan_seg_kind "index"); it serves plans of any window size and is freed here, so the data set
 * must outlive its plans as before.  Device memory: at most 0.25 B/SNP plus a few words per chromosome.
 * Wrapped device arrays (sfs2d_data_wrap_device) get none: their contents are the caller's and may be written
 * after a plan is created, in stream order ahead of a run; their plans read the positions on every pass. */
int sfs2d_data_free(sfs2d_data* data);

/* Synthetic sims replicates generated in HBM (BASELINE config 4: sims_scan.likelihood_scan's
 * replicate VCFs, sims_scan.py:593-644, at thousands of replicates).  Each replicate is one
 * chromosome of n_windows fixed windows of window_bp; win_snps[r * n_windows + w] (host) SNPs in
 * window w of replicate r (the caller draws them, e.g. Poisson(358.5)); per-SNP values from a
 * counter-based Philox stream keyed by seed and generation (the model is in sfs2d_kernels.hpp;
 * the host twin sfs2d.synth.sims_host reproduces it bit for bit).  miss_cdf1 / miss_cdf2: u32
 * inverse-CDF thresholds of the missing-allele counts of each population (nm entries, the last
 * 0xffffffff).  The data set owns its arrays. */
typedef struct {
  uint64_t seed;
  uint32_t generation, n_replicates, n_windows, window_bp;
  int32_t n1p, n2p;   /* diploid pop sizes: counts <= 2 * pop size */
} sfs2d_synth_params;
int sfs2d_data_synth_sims(sfs2d_ctx* ctx, const sfs2d_synth_params* sp, const uint16_t* win_snps,
                          const uint32_t* miss_cdf1, int32_t nm1, const uint32_t* miss_cdf2, int32_t nm2,
                          sfs2d_data** out);
/* copy a data set's packed counts / positions to host (n = the data set's SNP count; NULL skips) */
int sfs2d_data_read(const sfs2d_data* data, uint32_t* counts, uint32_t* pos, int64_t n);

/* Background SFS histograms of chromosome `chrom` (-1: all SNPs of the data set), with the
 * params' filters (position, variant_type, fold).  h2d: (2n1p+1)*(2n2p+1) int64, row-major
 * (alt1, alt2); h1a / h1b: UNFOLDED 1D spectra of raw alt counts, 2*pop_size+1 int64 each. */
int sfs2d_bg_hist(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, int32_t chrom,
                  int64_t* h2d, int64_t* h1a, int64_t* h1b);

/* The same histograms as ONE int64 row on the device (d_row: SFS2D_BG_ROW_WORDS int64), laid out
 * [2D bins | unfolded pop-1 spectrum | unfolded pop-2 spectrum | inner 2D sum (bins[1:-1])]: the
 * multi-GPU calculate_2d_sfs / calculate_1d_sfs (sfs2d/dist.py sharded_bg_hist) all-reduce these
 * rows over the ranks without a host copy.  Enqueued on the ctx stream; synchronises to report
 * SFS2D_E_KEY / SFS2D_E_GRID (the row is then undefined). */
#define SFS2D_BG_ROW_WORDS(n1p, n2p) ((2 * (n1p) + 1) * (2 * (n2p) + 1) + 2 * (n1p) + 2 * (n2p) + 3)
int sfs2d_bg_hist_dev(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, int32_t chrom,
                      int64_t* d_row);

/* Plans: everything that depends only on (data, params) is built once; plan_run enqueues the pass's
 * kernels (k_prep, k_bg_slice, the scan) with inputs and outputs resident in HBM. */
int sfs2d_plan_create(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, sfs2d_plan** out);
/* number of output records the plan writes (window slots, +1 when SFS2D_F_PREV_EXTRA) */
int64_t sfs2d_plan_num_records(const sfs2d_plan* plan);
/* SFS2D_BG_SUPPLIED: background values (host doubles, integer or normalised): bg2d has
 * (2n1p+1)*(2n2p+1) entries, bg1a / bg1b have n1p+1 / n2p+1 entries read at keys 1..pop_size-1
 * (folded or, for the sims path, unfolded spectra: quirk Q7). */
int sfs2d_plan_set_background(sfs2d_plan* plan, const double* bg2d, const double* bg1a, const double* bg1b);
/* enqueue the scan; out_dev: device buffer of sfs2d_plan_num_records records (NULL = plan-owned) */
int sfs2d_plan_run(sfs2d_plan* plan, sfs2d_window* out_dev);
/* enqueue `nruns` back-to-back runs (no host work in between; benchmarks and batch replays) */
int sfs2d_plan_run_many(sfs2d_plan* plan, int nruns, sfs2d_window* out_dev);
/* enqueue `nruns` runs round-robin over `nplans` distinct plans of one ctx: run i is plans[i % nplans]
 * on streams[i % nplans] (NULL = the HIP null stream, as sfs2d_ctx_set_stream) into outs[i % nplans]
 * (outs NULL or an entry NULL = plan-owned).  Independent scans (replicates, data sets, repeated
 * passes) overlap across the streams; each plan's own runs stay ordered on its stream.  The
 * ctx stream is unchanged after.  The runs are only enqueued: synchronise the passed streams before
 * sfs2d_plan_read / _check / _fst_read / _destroy of these plans (those synchronise the ctx stream
 * only). */
int sfs2d_plan_run_streams(sfs2d_plan* const* plans, void* const* streams, sfs2d_window* const* outs, int nplans,
                           int nruns);
/* the same run sequence captured once into HIP graphs, one per distinct stream (that stream's runs in
 * sequence order), and replayed by sfs2d_graph_launch: one hipGraphLaunch per stream and replay instead of
 * a launch per kernel (short passes are host-bound otherwise).  nruns must be a multiple of 2 * nplans
 * (every plan runs an even number of times per replay, so its buffer parity is unchanged); streams
 * non-null; no plan with timing on or attached.  The outputs are fixed at capture.  Replays run on the
 * capture streams, each after that stream's earlier work, without run_streams' staggered start.  A launch
 * fails with SFS2D_E_ARG when a captured plan ran an odd number of times since the capture.
 * The capture enqueues nothing for execution: it leaves every plan's last run, and where that run's records are,
 * as they were, and a plan that was created and captured but never run or replayed has NO last run (sfs2d_plan_read,
 * _fst_read and the post-scan calls refuse it like a plan that has not run).  A replay counts: after
 * sfs2d_graph_launch the last run of every captured plan (and of the plans attached to it) is its last run of the
 * replay, its records where the capture's outs put them, and sfs2d_plan_read, _fst_read, sfs2d_plan_null_run(_blocks),
 * _diversity, _spectra and _project work on it once the capture streams are synchronised (the launch only enqueues and
 * keeps host-side count of the runs; it synchronises nothing).  Not a
 * reference interface: repeated scans of the same data (the bench's loops; replicate loops as
 * sims_scan.py:593-644). */
int sfs2d_graph_create(sfs2d_plan* const* plans, void* const* streams, sfs2d_window* const* outs, int nplans,
                       int nruns, sfs2d_graph** out);
int sfs2d_graph_launch(sfs2d_graph* graph, int nlaunch);
int sfs2d_graph_destroy(sfs2d_graph* graph);
/* copy the last run's records to host (synchronises the stream).  The last run is the last one enqueued for
 * execution, however it was enqueued: sfs2d_plan_run (its out_dev or the plan's own buffer), _run_many, _run_streams,
 * phases 1 + 2 of sfs2d_plan_run_phase, sfs2d_plan_time, or a replay by sfs2d_graph_launch (the capture's outs).
 * SFS2D_E_ARG: a plan that has not run -- a capture alone is not a run */
int sfs2d_plan_read(sfs2d_plan* plan, sfs2d_window* out_host, int64_t cap, int64_t* nrec_out);
/* device pointers of the plan's per-chromosome background histogram replicas (uint32), for a
 * multi-GPU all-reduce between sfs2d_plan_run_phase(plan, 1) and (plan, 2). */
int sfs2d_plan_bg_buffer(sfs2d_plan* plan, void** dev_ptr, int64_t* nbytes);
/* Multi-GPU split of a chromosome over ranks (sfs2d/dist.py): between sfs2d_plan_run_phase(plan, 1)
 * (k_prep: this rank's part of every chromosome's background histograms) and (plan, 2) (tables and
 * scan), every rank reads its partial histograms -- replicas x nchrom x bins uint32 words, laid out
 * [replica][chromosome][bin] (the consumer sums the replicas), and nchrom uint32 per-chromosome inner
 * 2D sums (sizes: sfs2d_plan_bg_words) -- sums them over the ranks (the SURVEY 8(e) all-reduce) and
 * writes the totals back (to_device = 1).  Synchronous.  Replaces the whole-chromosome background
 * loops of calculate_2d_sfs / calculate_1d_sfs (twoDSFS_class.py:140-232, 398-444) when one
 * chromosome's SNPs are held by several ranks.  Plans without per-chromosome backgrounds: all 0. */
int sfs2d_plan_bg_words(const sfs2d_plan* plan, int64_t* replicas, int64_t* nchrom, int64_t* bins);
int sfs2d_plan_bg_exchange(sfs2d_plan* plan, uint32_t* host_repl, uint32_t* host_sums, int to_device);
/* The device-resident form of that exchange (no host copy; the SURVEY 8(e) all-reduce runs on the
 * rows in HBM, RCCL over xGMI): after sfs2d_plan_run_phase(plan, 1), _bg_rows_dev writes the plan's
 * per-chromosome partial histograms as int64 rows (row c at d_rows + c * row_stride, row_stride >=
 * SFS2D_BG_ROW_WORDS; layout of sfs2d_bg_hist_dev); after the all-reduce, _bg_rows_set_dev writes the
 * summed rows back (sums >= 2^32: SFS2D_E_ARG from sfs2d_plan_check), then sfs2d_plan_run_phase(plan, 2).
 * Both are enqueued on the ctx stream (order the collective against it). */
int sfs2d_plan_bg_rows_dev(sfs2d_plan* plan, int64_t* d_rows, int64_t row_stride);
int sfs2d_plan_bg_rows_set_dev(sfs2d_plan* plan, const int64_t* d_rows, int64_t row_stride);
/* Fst of the last run (as sfs2d_plan_read defines it) per window slot (NaN: no qualifying SNP / empty slot); plans
 * with SFS2D_F_FST; SFS2D_E_ARG: a plan that has not run */
int sfs2d_plan_fst_read(sfs2d_plan* plan, double* out_host, int64_t cap);
int sfs2d_plan_fst_buffer(sfs2d_plan* plan, void** dev_ptr, int64_t* nslots);
/* Fst output of the following runs: a caller-owned device buffer of >= nslots doubles (NULL = the plan-owned
 * buffer again), as sfs2d_plan_run's out_dev is for the records -- consecutive runs of one plan can keep their
 * Fst columns apart (e.g. each pass's table gathered while the next pass runs: bench.py at N > 1).  Attached
 * plans keep their own buffer. */
int sfs2d_plan_set_fst_out(sfs2d_plan* plan, double* d_fst);
int sfs2d_plan_run_phase(sfs2d_plan* plan, int phase, sfs2d_window* out_dev);
/* Multi-resolution: attach to `base` (a per-chromosome-background plan on the small-grid path) a
 * plan over the same data whose params differ only in window_mode / window / flags.  The base's
 * run then makes ONE k_prep pass over the SNP stream (background histograms, per-SNP bins, the
 * base's segmentation and Fst sums) and scans every attached plan from it before its own scan:
 * fixed-bp windows get their slots by binary search on the resident positions, SNP-count windows
 * need none; SFS2D_F_FST on an attached plan needs a fixed-bp Fst base whose window divides the
 * attached window (the base's per-window int64 fixed-point sums add exactly).  The reference
 * script scans the same data at 20 kb, 500 kb and 500 / 300 SNPs (twoDSFS_class.py:1923-2032).
 * An attached plan is not run on its own (its run calls fail); read it with sfs2d_plan_read /
 * sfs2d_plan_fst_read after the base's run.  Destroying the base destroys its attached plans. */
int sfs2d_plan_attach(sfs2d_plan* base, const sfs2d_params* params, sfs2d_plan** out);
/* Sliding windows: a fixed-bp plan (params->window_mode == SFS2D_WINDOW_BP) whose windows of W =
 * params->window bp advance by `step` bp instead of W: W % step == 0, 1 <= step <= W, W / step <= 64.  A
 * chromosome with last position L has (L - 1) / step + 1 slots (one when L == 0); slot j holds the SNPs
 * with j step + 1 <= pos <= j step + W (pos 0: slot 0 only).  The record's wid is j, begin / end its SNP
 * range; a slot without SNPs is an SFS2D_W_EMPTY record.  Filters keep their meaning (SFS membership,
 * not geometry); a per-chromosome background is the whole chromosome, counted once.  With step == W the
 * plan is the ordinary one (records and Fst byte-equal).  The plan is used like any other: sfs2d_plan_run,
 * _run_many, _run_streams, _read, _fst_read (every sliding plan with SFS2D_F_FST produces Fst), _check,
 * timing, sfs2d_graph_*.  SFS2D_F_PREV_EXTRA (quirk Q9 of the disjoint window loop), SNP-count windows
 * and a bad step are SFS2D_E_ARG, the reason in sfs2d_last_error.
 * The reference has no sliding scan: its script scans the same data twice, at 20 kb and at 500 kb, and
 * compares (twoDSFS_class.py:1923-1932), because a signal that straddles an edge of its disjoint
 * windows is split between two of them; overlapping windows are what that double scan stands in for. */
int sfs2d_plan_create_sliding(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, int64_t step,
                              sfs2d_plan** out);
/* The same as an attached plan (the rules of sfs2d_plan_attach; `base` is an ordinary or a sliding
 * plan): several window sizes, sliding by one step, from ONE k_prep pass of the base -- the 20 kb +
 * 500 kb pair of twoDSFS_class.py:1923-1932 as two sliding scans of one read of the SNP stream.  Fst of
 * an attached sliding plan needs nothing of the base (no Fst flag, no dividing window). */
int sfs2d_plan_attach_sliding(sfs2d_plan* base, const sfs2d_params* params, int64_t step, sfs2d_plan** out);
/* Region windows: a fixed-bp plan (params->window_mode == SFS2D_WINDOW_BP) whose windows
 * are the caller's n intervals instead of tiles placed by a rule -- genes, an inversion, candidate regions.
 * Region i is (chrom[i], first[i], last[i]): chrom an index into the data set's chromosomes, first <= last
 * 1-based inclusive positions below 2^32.  It holds the SNPs of that chromosome with first <= pos <= last:
 * begin = the chromosome's first SNP with pos >= first, end = the first with pos >= last + 1 (in 64 bits:
 * last = 2^32 - 1 is legal); repeated positions at a boundary are all inside; a SNP at pos 0 is inside only
 * when first == 0.  Regions may overlap, nest, repeat and come in any order within a chromosome, but chrom must
 * be non-decreasing over the list (a chromosome's slots are contiguous); a chromosome may have no region, and a
 * region may lie on a chromosome without SNPs.  Region i is slot i and record i: chrom its chromosome, wid its
 * index within the chromosome's regions, begin / end as above, an empty range an SFS2D_W_EMPTY record.  The three
 * arrays are HOST arrays, copied to the device once; n >= 1 and n < 2^31.  params->window is not geometry here
 * (any legal value): the plan's copy holds the longest region's length last - first + 1 (2^32 - 1 for the one
 * length above it).  Filters keep their meaning (SFS membership, not geometry); a per-chromosome background is
 * the whole chromosome, counted once, whether or not regions cover it.  Everything else is a sliding plan's:
 * sfs2d_plan_run, _run_many, _run_streams, _read, _fst_read (every regions plan with SFS2D_F_FST produces Fst),
 * _check, timing, sfs2d_graph_*, sfs2d_plan_diversity, sfs2d_plan_null_run(_blocks); sfs2d_plan_seg_kind says
 * "regions".  The 2D bins in LDS are 16-bit when no region holds 65,536 SNPs or more, counted exactly from the
 * library's host copy of the positions (sfs2d_data_upload); wrapped device arrays always take 32-bit bins.
 * SFS2D_E_ARG, the reason in sfs2d_last_error: a null array, n < 1, n >= 2^31, chrom out of range or decreasing,
 * first > last, SFS2D_F_PREV_EXTRA, SNP-count windows.
 * The reference has no such scan, nor anything in its place: it writes tiled windows (twoDSFS_class.py:787-991)
 * and its users cut the intervals they care about out of those tables afterwards. */
int sfs2d_plan_create_regions(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, const int32_t* chrom,
                              const uint32_t* first, const uint32_t* last, int64_t n, sfs2d_plan** out);
/* The same as an attached plan (the rules of sfs2d_plan_attach_sliding; `base` is an ordinary, a sliding or a
 * regions plan): the tiled scan and the per-region records from ONE k_prep pass of the base.  Its Fst needs
 * nothing of the base.  An ordinary plan attached to a regions base is treated as one attached to a sliding base. */
int sfs2d_plan_attach_regions(sfs2d_plan* base, const sfs2d_params* params, const int32_t* chrom,
                              const uint32_t* first, const uint32_t* last, int64_t n, sfs2d_plan** out);
/* Bootstrap null of T2D / T1D: how large is a window's T under "this window is a random
 * sample of its background"?  A task is a pair (pool, m): pool = a chromosome index c, meaning the SNPs
 * [chrom_off[c], chrom_off[c+1]) of the plan's data set, or -1, all of them (every SNP of the range, whatever
 * the filters: a drawn SNP carries its own classification and still counts toward m, as end - begin does for
 * a real window); m >= 1 SNPs are drawn from it with replacement, `replicates` times.  Draw j of replicate r:
 * c = philox4x32(counter (j >> 1, r, m, pool + 1), key (seed & 0xffffffff, seed >> 32)); x64 = c.x | c.y << 32
 * for even j, c.z | c.w << 32 for odd j; SNP index = lo + mulhi64(x64, n) (lo, n: the pool's first index and
 * size) -- a function of (seed, pool, m, r, j) alone, whatever the order or split of the tasks.  Record
 * t * replicates + r is replicate r of task t, evaluated as the scan's exact path evaluates a window, against
 * the background the plan uses for the pool (SFS2D_BG_PER_CHROM: table `pool`, pool -1 refused;
 * SFS2D_BG_SUPPLIED: the supplied table, any pool): chrom = pool (0xffffffff for -1), wid = r, begin = 0,
 * end = m, the counts, SFS2D_W_BG*_ZERO flags and T's as the scan writes them.  The drawn windows are never
 * stored.  tasks: ntasks (pool, m) pairs on the host; out_dev: ntasks * replicates records on the device
 * (NULL = plan-owned, read with sfs2d_plan_null_read).  Enqueued on the ctx stream after the plan's last run,
 * which it leaves as it found it (the next run's records and Fst are byte-equal).  The last run is sfs2d_plan_read's:
 * however it was enqueued, a replay by sfs2d_graph_launch included (the null completes the background tables again
 * after every replay, as after every run), and after a phase-split run the backgrounds are the exchanged rows; a
 * plan that was only captured has not run.  SFS2D_E_ARG, with the
 * reason in sfs2d_last_error: a plan that has not run, an attached plan (use its base: same data, same
 * tables), a pool out of range, pool -1 on a per-chromosome plan, an empty pool, m < 1, replicates < 1;
 * SFS2D_E_CAP: more than 2^26 records in one call, or sfs2d_plan_null_read's cap below the record count.
 * The reference has no null: its R script thresholds windows by SNP-count quantile and top 1 %
 * (ECBstats_plots.R:45-50, 147-219). */
typedef struct { uint64_t seed; uint32_t replicates; } sfs2d_null_params;
int sfs2d_plan_null_run(sfs2d_plan* plan, const sfs2d_null_params* np, const int64_t* tasks, int64_t ntasks,
                        sfs2d_window* out_dev);
/* The block null: sfs2d_plan_null_run (its last run and its refusals included) with runs of consecutive SNPs resampled instead of single SNPs, so that a
 * replicate window keeps the linkage of its pool ("blocks").  One block length `block` for
 * the call, 1 <= block < 2^32.  Task (pool, m), pool range [lo, lo + n), replicate r: nblk = ceil(m / block)
 * blocks; block i starts at s_i = mulhi64(x64, n), x64 being what draw i of sfs2d_plan_null_run uses
 * (c = philox4x32((i >> 1, r, m, pool + 1), key); c.x | c.y << 32 for even i, c.z | c.w << 32 for odd i: the block
 * length is not part of the counter); draw j = i * block + k (0 <= k < block, j < m) is SNP
 * lo + (s_i + k) mod n.  The pool is circular (every SNP keeps its marginal probability; pool -1 is one circle
 * over all chromosomes), the last block is cut at m, a block longer than the pool goes round it.  block == 1 is
 * sfs2d_plan_null_run itself (the same kernel, byte-equal records); any block >= m is one run of m consecutive
 * SNPs: a random placement of a window of m SNPs on the pool.  A record is a function of (seed, pool, m, block,
 * r) alone.  Everything else -- tasks, pools, backgrounds, the record layout, out_dev, sfs2d_plan_null_read, the
 * refusals and caps -- is sfs2d_plan_null_run's; in addition SFS2D_E_ARG for block < 1 or block >= 2^32. */
int sfs2d_plan_null_run_blocks(sfs2d_plan* plan, const sfs2d_null_params* np, int64_t block, const int64_t* tasks,
                               int64_t ntasks, sfs2d_window* out_dev);
int sfs2d_plan_null_read(sfs2d_plan* plan, sfs2d_window* out_host, int64_t cap, int64_t* nrec_out);
/* Per-window diversity: what kind of window a T2D / Fst peak is.  One record per record of
 * the plan's last run, at the same index; every field is a SUM over the window's SNPs (per-site values are the
 * caller's: sfs2d/diversity.py divides by the window length).  The SNPs are those of the record's own range
 * [begin, end) that are in the window's 2D SFS (the plan's position / variant_type filters, the joint fold); the
 * SNPs the SFS drops as bin (0, 0) are fixed for one allele in both populations and add exactly 0 to every field.
 * Per SNP, population k with counts (r, a), n = r + a called alleles:
 *   pi_k   += 2 a r / (n (n - 1))        (n >= 2; a fixed site adds exactly 0.0)
 *   s_k    += 1 when 0 < a < n           (segregating in k)
 *   thw_k  += [0 < a < n] / h(n),  h(n) = sum_{i=1}^{n-1} 1 / i      (Watterson, per SNP's own sample size)
 *   dxy    += (a1 r2 + r1 a2) / (n1 n2)  (n1, n2 >= 1)
 *   s_k_full, ar_k_full: s_k and the integer a r over the SNPs FULLY called in k (n == 2 pop_size_k exactly; a SNP
 *   with missing or surplus calls is not): Tajima's D is defined for one sample size, so it is formed from these
 *   (n = 2 pop_size_k, S = s_k_full, pi = 2 ar_k_full / (n (n - 1))) on the host.
 * flags: SFS2D_W_EMPTY / SFS2D_W_EXTRA of the source record; such a record has every other field 0.
 * The first member is a double (sfs2d_window is the record struct that begins with a uint32_t). */
typedef struct {
  double pi1, pi2, dxy, thw1, thw2;
  uint64_t ar1_full, ar2_full;
  uint32_t s1, s2, s1_full, s2_full, flags, reserved;
} sfs2d_diversity;
/* enqueue the diversity sums of the plan's last run (its records: sfs2d_plan_run's out_dev or the plan's own) on
 * the ctx stream; out_dev: device buffer of sfs2d_plan_num_records records (NULL = plan-owned, read with
 * sfs2d_plan_diversity_read).  Any plan that has run, attached plans included (their own records, their base's
 * data); reads the records, the counts and (filtered plans) the per-SNP bins, writes out_dev alone: a following
 * run or null run finds everything as it was.  The last run is sfs2d_plan_read's (a replay by sfs2d_graph_launch
 * counts, a capture alone does not).  SFS2D_E_ARG, with the reason in sfs2d_last_error: a plan that
 * has not run.  The reference has no such statistic (its users join pixy's or scikit-allel's by window label). */
int sfs2d_plan_diversity(sfs2d_plan* plan, sfs2d_diversity* out_dev);
/* copy the last sfs2d_plan_diversity call's records to host (synchronises); SFS2D_E_CAP: cap below the record
 * count (*nrec_out holds it); SFS2D_E_ARG: no diversity call since the plan was created */
int sfs2d_plan_diversity_read(sfs2d_plan* plan, sfs2d_diversity* out_host, int64_t cap, int64_t* nrec_out);
/* Window spectra: the joint and folded 1D spectra themselves of chosen records of the plan's
 * last run, summed into groups -- what the scan reduces to T2D / T1D and four totals per window, as the x_k.  For
 * a record with SNP range [begin, end) (clamped to the data set's SNP count), under the plan's position filter,
 * variant_type filter and fold:
 *   2D   the dense (2 n1p + 1) x (2 n2p + 1) grid of calculate_2d_sfs over the window, row-major (x1, x2); bin (0, 0)
 *        is 0 (the reference skips those SNPs), the last bin (n1, n2) is counted
 *   1D   per population the folded spectrum of raw alt counts at the inner bins 1 .. pop_size - 1, the bins T1D
 *        reads; entries 0 and pop_size are 0
 * A group's row is SFS2D_SPEC_ROW_WORDS int64, laid out [2D bins | pop-1 folded, n1p + 1 | pop-2 folded, n2p + 1],
 * the sum over the group's selection entries: a record listed twice is counted twice, a group with no entry is all
 * 0, entries that name an SFS2D_W_EMPTY or SFS2D_W_EXTRA record add nothing.  On overlapping windows (sliding,
 * regions) a group is the SUM over its windows, not the spectrum of their union: a SNP in two selected windows is
 * counted twice.
 * rec / grp: nsel (record index, group) pairs, HOST arrays copied to the device by the call, in any order
 * (consecutive entries of one group are cheapest).  rec == NULL with nsel == sfs2d_plan_num_records: every record in
 * order; then grp == NULL: group i = record i.  out_dev: ngroups rows on the device (NULL = plan-owned, read with
 * sfs2d_plan_spectra_read), zeroed by the call.  Enqueued on the ctx stream after the plan's last run; any plan that
 * has run, attached, sliding, regions and SNP-count plans included (their own records, the base's data and bins).
 * Reads the records, the counts and (filtered plans) the per-SNP bins, writes out_dev alone: a following run, null
 * run or diversity call finds everything as it was.  Integer sums: two calls give byte-equal rows.  The last run is
 * sfs2d_plan_read's (a replay by sfs2d_graph_launch counts, a capture alone does not).
 * SFS2D_E_ARG, the reason in sfs2d_last_error: a plan that has not run, nsel < 0, ngroups < 1, a record index
 * outside [0, nrec), a group outside [0, ngroups), grp == NULL with rec != NULL, rec == NULL with nsel != nrec;
 * SFS2D_E_NOMEM: ngroups rows do not fit.
 * The reference merges the outlier windows' SNPs into new VCFs with an outside tool and runs calculate_2d_sfs on
 * them again (sims_scan.py:726-936). */
#define SFS2D_SPEC_ROW_WORDS(n1p, n2p) ((2 * (n1p) + 1) * (2 * (n2p) + 1) + (n1p) + (n2p) + 2)
int sfs2d_plan_spectra(sfs2d_plan* plan, const int64_t* rec, const int32_t* grp, int64_t nsel, int64_t ngroups,
                       int64_t* out_dev);
/* copy the last sfs2d_plan_spectra call's rows to host (synchronises); *nwords_out: ngroups x row words;
 * SFS2D_E_CAP: cap_words below it; SFS2D_E_ARG: no spectra call since the plan was created */
int sfs2d_plan_spectra_read(sfs2d_plan* plan, int64_t* out_host, int64_t cap_words, int64_t* nwords_out);
/* Projected window spectra: the joint spectrum of chosen records of the plan's last run,
 * projected down hypergeometrically to the haploid sample sizes (m1, m2), 2 <= m_k <= 2 pop_size_k, and summed into
 * groups -- what a model fit (dadi, moments, fastsimcoal) takes when calls are missing: sfs2d_plan_spectra bins a
 * SNP by its raw alt count whatever its called count.  For a record with SNP range [begin, end) (clamped to the data
 * set's SNP count):
 *   member   a SNP that the plan's run counts in its 2D SFS (the position and variant_type filters, no (0, 0) SNPs)
 *   used     a member with called counts n1 = r1 + a1 >= m1 and n2 = r2 + a2 >= m2 (surplus calls, n_k > 2 pop_size_k,
 *            included); any other member is dropped
 *   grid     a used SNP adds h(j1; n1, a1, m1) h(j2; n2, a2, m2) to bin (j1, j2) of the dense (m1 + 1) x (m2 + 1)
 *            grid, row-major, with h(j; n, a, m) = C(a, j) C(n - a, m - j) / C(n, m) on its support
 *            max(0, m - (n - a)) <= j <= min(m, a).  The RAW alt counts are projected; nothing is folded (the fold,
 *            the marginals and their folds are linear: sfs2d/spectra.py forms them on the host).
 * A group's row is SFS2D_PROJ_ROW_WORDS int64, laid out [grid, fixed point 2^-e | n_used | n_dropped], summed over
 * the group's selection entries by sfs2d_plan_spectra's rules (a record listed twice counts twice, EMPTY and EXTRA
 * records add nothing, a group without entries is all 0, overlapping windows are summed, not united).  Each term is
 * rounded to nearest at 2^-e once and the sums are integer: two calls give byte-equal rows.  e is chosen per call,
 * e = min(40, 62 - bitlen(B)), B = the largest number of entries of one group x the bound on an entry's SNPs (the
 * plan's bound on a window's SNPs; the longest named chromosome if that is more), and reported in *e_out (NULL:
 * not wanted).
 * rec / grp / nsel / ngroups / out_dev: as sfs2d_plan_spectra, NULL forms included, and in addition rec[i] = -(c + 1)
 * names the whole chromosome c of the plan's data set, [chrom_off[c], chrom_off[c + 1]), under the same membership:
 * a projected per-chromosome background on any plan kind.  Enqueued on the ctx stream after the plan's last run;
 * reads the records, the counts and (filtered plans) the per-SNP bins, writes out_dev alone: a following run, null
 * run, diversity or spectra call finds everything as it was.  The last run is sfs2d_plan_read's (a replay by
 * sfs2d_graph_launch counts, a capture alone does not).
 * SFS2D_E_ARG, the reason in sfs2d_last_error: a plan that has not run, m_k < 2 or m_k > 2 pop_size_k, a chromosome
 * outside [0, nchrom), and sfs2d_plan_spectra's refusals of the selection; SFS2D_E_NOMEM: ngroups rows do not fit;
 * SFS2D_E_CAP: B leaves fewer than 8 fraction bits.
 * The reference has no projection (its users extract the outlier windows' SNPs and run easySFS on them). */
#define SFS2D_PROJ_ROW_WORDS(m1, m2) (((m1) + 1) * ((m2) + 1) + 2)
int sfs2d_plan_project(sfs2d_plan* plan, int32_t m1, int32_t m2, const int64_t* rec, const int32_t* grp, int64_t nsel,
                       int64_t ngroups, int64_t* out_dev, int32_t* e_out);
/* copy the last sfs2d_plan_project call's rows to host (synchronises) as doubles, x * 2^-e: out_host ngroups x
 * (m1 + 1)(m2 + 1) grids, used / dropped ngroups counts each.  *ngroups_out, *words_per_group: the call's groups and
 * grid words; SFS2D_E_CAP: cap_groups below the former; SFS2D_E_ARG: no project call since the plan was created */
int sfs2d_plan_project_read(sfs2d_plan* plan, double* out_host, int64_t* used, int64_t* dropped, int64_t cap_groups,
                            int64_t* ngroups_out, int64_t* words_per_group);
/* the weights h(j; n, a, m), j = 0 .. m, into w_out (m + 1 doubles): host only, no device or ctx, the source the
 * kernel evaluates (ln k! table, one exp per weight; exactly 0 outside the support, exactly 1 on a support of one
 * bin).  SFS2D_E_ARG: a > n, m > n, n > 510, a negative argument or w_out == NULL */
int sfs2d_project_weights(int32_t n, int32_t a, int32_t m, double* w_out);
/* The projected scan: T2D, T1D_pop1 and T1D_pop2 of EVERY record of the plan's last run at the
 * common haploid sample size (m1, m2), 2 <= m_k <= 2 pop_size_k -- the scan's statistics without the pull toward the
 * low bins that missing calls give a window (the scan bins a SNP by its raw alt count whatever its called count).  One
 * record per record of the last run, at the same index.  Members, used and dropped SNPs, the weights and the fixed
 * point are sfs2d_plan_project's; per record:
 *   window grid X  the projected (m1 + 1) x (m2 + 1) grid of its SNP range [begin, end) (clamped to the data set),
 *                  folded jointly when the plan folds: bin (j1, j2) with 2 (j1 + j2) > m1 + m2 is added to
 *                  (m1 - j1, m2 - j2), a tie stays where it is; unfolded otherwise
 *   background b   the same grid over the whole chromosome the record's chrom names, under the same membership
 *                  (bg_chrom = -1), or over chromosome bg_chrom for every record (bg_chrom >= 0)
 *   t2d            2 sum_{x_k > 0} x_k (ln(x_k / N) - ln(b_k / B)), x = X.ravel()[1:-1], N = sum x, B = sum b[1:-1];
 *                  +inf when a touched bin has b_k = 0; NaN exactly when N = 0 or B = 0
 *   t1d_p1/_p2     the same form on the marginal of the grid folded min(j, m_k - j), at its inner bins 1 <= j,
 *                  2 j < m_k (bin 0 and, for even m_k, the bin at m_k / 2 are not read: at m_k = 2 pop_size_k these
 *                  are the bins 1 .. pop_size_k - 1 that T1D reads), against the chromosome's marginal
 *   n2_fx, n1a_fx, n1b_fx  the three N as integers at the fixed point 2^-e; n_used / n_dropped as sfs2d_plan_project
 *   flags          SFS2D_W_EMPTY / SFS2D_W_EXTRA of the source record; such a record has every other field 0
 * The statistic is the closed form above: the reference's exact 0.0 for proportional spectra and scipy's NaN rule for
 * an empty last bin are not reproduced (on fully called data at m_k = 2 pop_size_k it agrees with the scan's T to
 * rounding wherever that is finite and non-zero).  Every term of a grid is rounded to nearest once and the sums are
 * integer; the floating-point sums run in a fixed order: two calls give byte-equal records, however the records fall
 * to workgroups.  *e_out: the windows' fixed point, e = min(40, 62 - bitlen(the plan's bound on a window's SNPs)),
 * what sfs2d_plan_project reports for one record per group; *e_bg_out: the backgrounds', by sfs2d_plan_project's rule
 * for one chromosome entry per group (NULL: not wanted).  The window grids live in LDS alone (8 bytes per bin beside
 * the marginals and a 4 KB table): there is no global-memory variant.
 * out_dev: sfs2d_plan_num_records records on the device (NULL = plan-owned, read with sfs2d_plan_project_scan_read).
 * Enqueued on the ctx stream after the plan's last run (sfs2d_plan_read's: a replay by sfs2d_graph_launch counts, a
 * capture alone does not), nothing is read back; any plan that has run, attached, sliding, regions, SNP-count and
 * filtered plans and wrapped device data included.  Reads the records, the counts and (filtered plans) the per-SNP
 * bins, writes out_dev and its own buffers alone: a following run, null run, diversity, spectra or project call finds
 * everything as it was, and sfs2d_plan_project_read still reads the last sfs2d_plan_project call.
 * SFS2D_E_ARG, the reason in sfs2d_last_error: a plan that has not run, m_k < 2 or m_k > 2 pop_size_k, bg_chrom
 * outside [-1, nchrom), a plan with a supplied background (SFS2D_BG_SUPPLIED); SFS2D_E_CAP: a grid that does not fit
 * the 160 KB of LDS of a compute unit, fewer than 8 fraction bits; SFS2D_E_NOMEM.
 * The reference has no projection and scans raw alt counts (twoDSFS_class.py:787-991). */
typedef struct {
  double t2d, t1d_p1, t1d_p2;
  int64_t n2_fx, n1a_fx, n1b_fx;   /* N of T2D / T1D_pop1 / T1D_pop2, fixed point 2^-e */
  uint32_t n_used, n_dropped;
  uint32_t flags;                  /* SFS2D_W_EMPTY | SFS2D_W_EXTRA bits of the source record */
  uint32_t e;
} sfs2d_projstat;
int sfs2d_plan_project_scan(sfs2d_plan* plan, int32_t m1, int32_t m2, int32_t bg_chrom, sfs2d_projstat* out_dev,
                            int32_t* e_out, int32_t* e_bg_out);
/* copy the last sfs2d_plan_project_scan call's records to host (synchronises); SFS2D_E_CAP: cap below the record
 * count (*nrec_out holds it); SFS2D_E_ARG: no such call since the plan was created */
int sfs2d_plan_project_scan_read(sfs2d_plan* plan, sfs2d_projstat* out_host, int64_t cap, int64_t* nrec_out);
/* The null of the projected scan: replicates of chosen records of the plan's last run in which
 * every used SNP is replaced by one drawn among the used SNPs of its chromosome with the SAME called counts.  The
 * projected T still grows as a window's called counts approach (m1, m2) -- a SNP called in exactly m alleles adds an
 * indicator to the grid, one called in n > m a spread-out hypergeometric row -- so a null that keeps each window's
 * called counts is the one that can judge it; under missingness independent of frequency it is exact conditional on
 * the window's coverage.  (m1, m2), the last run, membership, "used" (member & n1c >= m1 & n2c >= m2), the weights,
 * the per-term rounding at 2^-e, the joint fold, the three statistics and their NaN / +inf rules are
 * sfs2d_plan_project_scan's.
 *   pool, stratum  the pool of chromosome c is its used SNPs; the stratum of a used SNP is the set of the pool's SNPs
 *                  with the same (n1c, n2c) (called alleles per population), in ascending SNP index; a SNP is in its
 *                  own stratum, so none is empty
 *   entry          a record index s = rec[t] of the last run (rec == NULL: every record, nsel = the record count);
 *                  each entry gets np->replicates = R replicates; output record t R + r is replicate r of entry t.  An
 *                  EMPTY / EXTRA source record gives R records with its flags and zeros
 *   slot i of replicate r  SNP k = begin + i of the record's clamped range.  A SNP that is not used draws nothing.  A
 *                  used SNP with stratum (start, size) in its chromosome's pool draws
 *                    c = philox4x32(counter (i >> 1, r, s, chrom + 1), key (seed & 0xffffffff, seed >> 32));
 *                    x64 = c.x | c.y << 32 for even i, c.z | c.w << 32 for odd i;
 *                    SNP pool_idx[start + mulhi64(x64, size)]
 *                  -- integers only, a function of (seed, s, r, i) and the data, whatever the launch geometry and
 *                  however a selection is split over calls
 *   record         what sfs2d_plan_project_scan would write for a window made of the drawn SNPs, against the record's
 *                  chromosome; *e_out / *e_bg_out are exactly those sfs2d_plan_project_scan reports for this plan and
 *                  (m1, m2); n_used / n_dropped are the window's
 *   thin           one uint32 per entry: the used slots whose stratum holds fewer than SFS2D_PNULL_THIN SNPs (such a
 *                  slot is redrawn from almost nothing, which narrows the null; reported, not acted on)
 * The pools (the SNPs sorted stably by chromosome and called counts, and a dense table of (start, size) per chromosome
 * and called-count pair) are built by the first call after a run or with another (m1, m2) and kept on the plan.
 * out_dev: nsel R records on the device; thin_dev: nsel uint32 (NULL = plan-owned, read with
 * sfs2d_plan_project_null_read).  Enqueued on the ctx stream; attached, sliding, regions, SNP-count and filtered plans
 * and wrapped device data as sfs2d_plan_project_scan.  Writes out_dev, thin_dev and its own buffers alone.
 * SFS2D_E_ARG, the reason in sfs2d_last_error: a plan that has not run, m_k < 2 or m_k > 2 pop_size_k, a plan with a
 * supplied background, replicates < 1, a record index outside the plan's records; SFS2D_E_CAP: more than 2^26 records
 * in one call, a grid that does not fit the LDS of a compute unit, fewer than 8 fraction bits; SFS2D_E_NOMEM.
 * A background chromosome for every record (a foreign pool can have empty strata), supplied backgrounds, block
 * bootstraps (strata break adjacency) and size classes (every window has its own null) are not offered. */
#define SFS2D_PNULL_THIN 8
int sfs2d_plan_project_null(sfs2d_plan* plan, int32_t m1, int32_t m2, const sfs2d_null_params* np, const int64_t* rec,
                            int64_t nsel, sfs2d_projstat* out_dev, uint32_t* thin_dev, int32_t* e_out, int32_t* e_bg_out);
/* copy the last sfs2d_plan_project_null call's records (out_host NULL: not wanted, cap is not read) and thin-slot
 * counts (thin_host NULL: not wanted) to host (synchronises); cap counts records; SFS2D_E_CAP: cap below the record count (*nrec_out holds it); SFS2D_E_ARG: no
 * such call since the plan was created */
int sfs2d_plan_project_null_read(sfs2d_plan* plan, sfs2d_projstat* out_host, uint32_t* thin_host, int64_t cap,
                                 int64_t* nrec_out);
/* launch geometry (threads per grid) of k_prep and of the scan kernel: matches the Grid_Size column
 * of rocprofv3 kernel traces, so profiles can be joined to a plan */
int sfs2d_plan_grids(const sfs2d_plan* plan, int64_t* prep_threads, int64_t* scan_threads);
/* name of the scan kernel the plan launches ("k_scan_w", "k_scan_gw", "k_scan_g"; the
 * prefix of its rocprofv3 kernel name), NULL for a null plan */
const char* sfs2d_plan_scan_kernel(const sfs2d_plan* plan);
/* where the plan's window slots come from: "prep" (k_prep's segmentation pass over the positions), "index"
 * (k_slots_index over the data set's position index, ahead of a k_prep that reads no positions: fixed-bp
 * counts plans with per-chromosome backgrounds over uploaded or generated data, unless SFS2D_SEG=prep at plan
 * creation), "search"
 * (k_slots_search), "synth" (the generator's window offsets), "slide" (k_slots_slide), "regions" (k_slots_regions), "bp" (an attached
 * fixed-bp plan: k_slots_bp), "none" (SNP-count windows); NULL for a null plan */
const char* sfs2d_plan_seg_kind(const sfs2d_plan* plan);
/* 1: the plan's slot table is written by its first run alone and later runs launch no slot kernel -- "index"
 * plans with Fst summed in the scan, whose scan never stores to the table (its inputs, the data set's position
 * index, the window and the slot bases, are fixed for the plan); 0: every run writes it (also with
 * SFS2D_SLOTS_ONCE=0 at plan creation); SFS2D_E_ARG for a null plan */
int sfs2d_plan_slots_once(const sfs2d_plan* plan);
/* template arguments of the scan kernel the plan's last run launched; -1 where the kernel has no such argument
 * (k_scan_w: p16, fused, fst 0..3, cnt, gate; k_scan_gw: p16, fst, cnt, tri; k_scan_g: p16, fst, cnt).  p16 == 0:
 * 32-bit 2D bins in LDS (a window may hold >= 65,536 SNPs).  An attached plan records at its own launch inside
 * its base's run.  SFS2D_E_ARG before any run (or when no run launched a scan kernel); NULL outputs are skipped */
int sfs2d_plan_scan_variant(const sfs2d_plan* plan, int* p16, int* fused, int* fst, int* cnt, int* gate, int* tri);
/* beside it, for k_scan_w plans (-1 each for the large-grid kernels): tri 1 when the plan launches k_scan_wt, the
 * lean variants on a triangle-packed window histogram (lean plans with n1 = n2, at least 8 windows per resident
 * wavefront and a workgroup within 80 KB of LDS; SFS2D_TRI=0 at plan creation keeps the lean variant, SFS2D_TRI=1
 * drops the windows-per-wavefront condition -- same results), sb the windows per batched finish
 * and r1 the lane copies of the 1D window histograms.  Known from plan creation.  SFS2D_E_ARG for a null plan */
int sfs2d_plan_scan_packing(const sfs2d_plan* plan, int* tri, int* sb, int* r1);
/* cumulative number of windows re-evaluated on the exact path (|T| ~ 0: proportionality test) */
int sfs2d_plan_stats(sfs2d_plan* plan, uint32_t* exact_windows);
/* last run's error word (0 = ok, else SFS2D_E_KEY / SFS2D_E_GRID, or SFS2D_E_ARG for summed background
 * rows that overflow); synchronises */
int sfs2d_plan_check(sfs2d_plan* plan);
/* live timing: every `every`-th of the following runs (up to `max_samples` of them) launches k_prep
 * and the scan kernel with start/stop events in their own dispatch packets (hipExtLaunchKernelGGL):
 * kernel start/end timestamps, the durations rocprofv3 --kernel-trace reports; no extra packets
 * between kernels.  sfs2d_plan_timing_read averages the sampled runs' per-kernel durations */
int sfs2d_plan_set_timing(sfs2d_plan* plan, int max_runs);   /* = sampled(plan, max_runs, 1) */
int sfs2d_plan_set_timing_sampled(sfs2d_plan* plan, int max_samples, int every);
/* the same for a subset of the kernels: bit 0 k_prep, bit 1 k_bg_slice, bit 2 the scan kernel (an event
 * pair costs queue time: the bench times only the scan kernel inside its timed loop); the kernels
 * left out read 0 in sfs2d_plan_timing_read */
int sfs2d_plan_set_timing_kernels(sfs2d_plan* plan, int max_samples, int every, int kernel_mask);
/* average device time per kernel over the sampled runs (synchronises): k1 = k_prep, k2 = k_bg_slice
 * (0 when the plan does not launch it), k3 = the window scan kernel (k_scan_w / k_scan_gw / k_scan_g) */
int sfs2d_plan_timing_read(sfs2d_plan* plan, int* nruns, double* ms_k1, double* ms_k2, double* ms_k3);
/* standalone timing loop: average device time per kernel over `iters` runs */
int sfs2d_plan_time(sfs2d_plan* plan, int iters, double* ms_per_run, double* ms_k1, double* ms_k2, double* ms_k3);
int sfs2d_plan_destroy(sfs2d_plan* plan);

/* one-shot convenience: plan + run + read (+ supplied background when bg2d != NULL) */
int sfs2d_scan(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, const double* bg2d,
               const double* bg1a, const double* bg1b, sfs2d_window* out_host, int64_t cap, int64_t* nrec_out);

#ifdef __cplusplus
}
#endif
#endif /* SFS2D_H */
