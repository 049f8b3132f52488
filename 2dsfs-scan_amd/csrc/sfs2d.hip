// sfs2d.hip -- host side + C ABI of the MI355X (gfx950) windowed 2D-SFS composite-likelihood scan.
//
// Device code lives in sfs2d_kernels.hpp (see its header for the statistic and the kernels).
// One run of a plan enqueues, on the context's stream:
//   k_prep         counts + positions (8 B/SNP) -> packed per-SNP bins (4 B/SNP), per-chromosome
//                  background histograms + inner sums, fixed-bp segmentation of the window slots
//   k_bg_slice     per-chromosome background tables (skipped for supplied backgrounds)
//   k_scan_w / _g  bins (4 B/SNP) -> one 64-B record per window slot
//   k_scan_extra   combined_scan's final-window helper (only with SFS2D_F_PREV_EXTRA)
// Sliding plans (sfs2d_plan_create_sliding) run k_prep without its segmentation, then k_slots_slide
// (the overlapping slot table by binary search), the tables, k_fst_win where the scan does not sum
// Fst itself, and the same scan kernels.
// After a run, sfs2d_plan_diversity enqueues k_div_win (sfs2d_div.hpp) over the run's records: per-window pi, dxy,
// Watterson and Tajima sums from the resident counts; it writes its own output alone.
// sfs2d_plan_spectra enqueues k_spec_win (sfs2d_spec.hpp) over chosen records of the run: their 2D and folded 1D
// spectra themselves, summed into groups, as int64 rows; it too writes its own output alone.
// sfs2d_plan_project enqueues k_proj_win (sfs2d_proj.hpp) over chosen records or whole chromosomes: the joint
// spectrum projected down to a common sample size, as int64 fixed-point rows; it writes its own output alone.
// sfs2d_plan_project_scan enqueues k_proj_win over the background chromosomes, k_proj_lp and k_proj_scan
// (sfs2d_projscan.hpp): T2D / T1D of every record at a common sample size, the window grids in LDS alone.
// sfs2d_plan_project_null builds, once per run and projection, the pools of used SNPs sorted by (chromosome, called
// counts) and their stratum table (k_pnull_keys, a stable radix sort, k_pnull_heads), then enqueues k_proj_null
// (sfs2d_projnull.hpp): replicates of chosen records whose SNPs are redrawn among SNPs of equal called counts.
// All device state a run touches (slot table, background replicas and counters, LDS) is left
// zeroed by the run itself, so plans replay without memsets.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "sfs2d.h"
#include "sfs2d_kernels.hpp"
#include "sfs2d_div.hpp"
#include "sfs2d_spec.hpp"
#include "sfs2d_proj.hpp"
#include "sfs2d_projscan.hpp"
#include "sfs2d_projnull.hpp"

// the pool build's stable sort (set-up of sfs2d_plan_project_null, not a hot path)
#include <rocprim/device/device_radix_sort.hpp>

using namespace sfs2dk;

namespace {

// numpy pairwise_sum recursion over n elements: n <= 128 -> leaf (np_leaf_sum), else split at
// n2 = n/2 - (n/2 % 8).  Leaves are numbered left to right; internal nodes get ids nleaves + i
// sorted by height (children before parents, the root last), with level = height - 1, so that a
// node can be combined as soon as its level is reached (same sums, same order inside each node).
struct PwTree {
  std::vector<int2> leaves;   // {offset, n}
  std::vector<int4> nodes;    // {child a, child b, level, 0} (leaf ids < nleaves, node ids >= nleaves)
  int nlevels = 0;
};

int pw_build(int lo, int n, PwTree& t, std::vector<int2>& raw, std::vector<int>& height) {
  // returns a provisional id: >= 0 leaf, < 0 internal node -(i+1)
  if (n <= 128) {
    t.leaves.push_back(make_int2(lo, n));
    return (int)t.leaves.size() - 1;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  const int a = pw_build(lo, n2, t, raw, height);
  const int b = pw_build(lo + n2, n - n2, t, raw, height);
  auto h = [&](int id) { return id >= 0 ? 0 : height[-id - 1]; };
  raw.push_back(make_int2(a, b));
  height.push_back(std::max(h(a), h(b)) + 1);
  return -(int)raw.size();
}

PwTree pw_plan(int n) {
  PwTree t;
  std::vector<int2> raw;
  std::vector<int> height;
  if (n > 0) pw_build(0, n, t, raw, height);
  const int L = (int)t.leaves.size();
  std::vector<int> order(raw.size());
  for (size_t i = 0; i < raw.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return height[x] < height[y]; });
  std::vector<int> newid(raw.size());
  for (size_t i = 0; i < order.size(); ++i) newid[order[i]] = L + (int)i;
  auto remap = [&](int id) { return id >= 0 ? id : newid[-id - 1]; };
  for (int i : order) {
    t.nodes.push_back(make_int4(remap(raw[i].x), remap(raw[i].y), height[i] - 1, 0));
    t.nlevels = std::max(t.nlevels, height[i]);
  }
  return t;
}

// (p-1)/ws as a multiply-high (Granlund-Montgomery, 33-bit magic): q = (t + ((n-t) >> s1)) >> s2
void div_magic(uint32_t d, uint32_t* m, int* s1, int* s2) {
  if (d <= 1) { *m = 0; *s1 = 0; *s2 = 0; return; }
  int l = 0;
  while ((1ull << l) < d) ++l;   // ceil(log2 d)
  *m = (uint32_t)((((unsigned __int128)1 << 32) * (((unsigned __int128)1 << l) - d)) / d + 1);
  *s1 = 1;
  *s2 = l - 1;
}

}  // namespace

// the stream the library enqueues on: the ctx's current one (sfs2d_ctx_set_stream)
#define CTX_STREAM(c) ((c)->stream)

struct sfs2d_ctx {
  int device = 0;
  int ncu = 256;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  double* d_lnx = nullptr;
  double* d_df = nullptr;   // D(r), F(x) (LNT each), then (1/k, 1/(k(k-1))) pairs (RCPN)
  double* d_lf = nullptr;   // ln k!, k < PROJ_LF: k_proj_win's weights (allocated by the first sfs2d_plan_project)
  double* d_hw = nullptr;   // 1 / h(n), h(n) = sum_{i=1}^{n-1} 1/i, for n < RCPN (0 below n = 2): k_div_win's Watterson terms
  hipEvent_t stagger = nullptr;   // sfs2d_plan_run_streams: the first run's k_prep, awaited by the second stream
  bool capturing = false;         // sfs2d_graph_create is capturing: the runs it enqueues execute at sfs2d_graph_launch
  std::string err;
  std::mutex err_mu;
};

struct sfs2d_data {
  sfs2d_ctx* ctx = nullptr;
  bool owned = false;
  uint32_t* counts = nullptr;
  uint32_t* pos = nullptr;
  uint16_t* ann = nullptr;
  long long* d_chrom_off = nullptr;
  int64_t n = 0;
  int32_t nchrom = 0;
  std::vector<int64_t> chrom_off;
  std::vector<uint32_t> last_pos;
  std::vector<uint32_t> host_pos;   // upload path only: exact window-length bound for u16 bins
  bool ann_owned = false;
  bool strict = true;   // positions strictly increasing within each chromosome
  // the largest called allele counts r + a of population 1 / 2 over the data set: counts plans with a
  // supplied background run no pass that validates the counts (k_prep reads none), so they need
  // max_nc1 <= n1 and max_nc2 <= n2 -- then no SNP can raise KeyError (a > 2 pop_size) or leave the
  // grid after the fold; otherwise the plan takes the bins pipeline, whose k_prep raises the error
  uint32_t max_nc1 = 0xffffffffu, max_nc2 = 0xffffffffu;
  // some SNP has fewer than 2 called alleles in a population (unknown: true): Fst summed in the scan
  // must then drop such SNPs explicitly (k_scan_w<..., 3, ...>); without any, the unmasked terms are exact
  bool low_nc = true;
  // sfs2d_data_synth_sims: the generator's window offsets (SNP index of window w's first SNP, nwin + 1
  // entries; w = replicate * win_per_chrom + window), its window length and windows per replicate --
  // fixed-bp plans of that window length take their slot table from them instead of k_prep's
  // segmentation pass over the positions (the generator placed window w's SNPs in its own window)
  unsigned long long* d_win_off = nullptr;
  uint32_t win_bp = 0, win_per_chrom = 0;
  // the position index (k_pos_index; data_pos_index builds it when the first plan that wants it is created,
  // for a data set whose positions the library owns -- an upload, generated replicates; it serves plans of any
  // window size and is freed with the data set): d_pidx the entries, d_pidx_base nchrom + 1 entry bases, d_pidx_sh nchrom cell shifts
  mutable std::mutex pidx_mu;
  mutable uint32_t* d_pidx = nullptr;
  mutable uint32_t* d_pidx_base = nullptr;
  mutable uint32_t* d_pidx_sh = nullptr;
};

// A grow-on-demand device array of a post-scan call (reserve) and a call's result (call_out, read_last): the
// plan-owned buffer, where the last call wrote -- that buffer or the caller's -- and how many elements; NONE: no
// call yet.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;   // elements
};
template <typename T, int64_t NONE = -1>
struct CallOut {
  DevBuf<T> own;
  const T* last = nullptr;
  int64_t n = NONE;
};

struct sfs2d_plan {
  sfs2d_ctx* ctx = nullptr;
  const sfs2d_data* data = nullptr;
  sfs2d_params prm{};
  KParams K{};
  int nbg = 0;
  bool do_bg = false, do_seg = false, lds_hist = true, bg_ready = false;
  bool seg_synth = false;   // fixed-bp slots from the generator's window offsets (slots_only)
  bool seg_search = false;  // fixed-bp slots by binary search on the positions, k_slots_search (slots_only)
  bool seg_index = false;   // fixed-bp slots from the data set's position index, k_slots_index ahead of a k_prep
                            // that does not segment (counts plans with per-chromosome backgrounds)
  // seg_index plans whose scan never stores to the slot table (Fst summed in the scan): the table depends on
  // the position index, the window and the slot bases alone, all fixed for the plan, so the plan's first run
  // writes it and later runs launch no slot kernel (stage_slots)
  bool slots_once = false, slots_written = false;
  int64_t step = 0;         // sliding plan: fixed-bp windows advanced by step bp (0: disjoint windows); its
                            // slots by k_slots_slide, k_prep without segmentation
  bool regions = false;     // regions plan: slot s is the caller's interval s (d_reg), its slots by k_slots_regions
                            // where a sliding plan launches k_slots_slide; everything else as a sliding plan
  uint2* d_reg = nullptr;   // the regions' (first, last), 1-based inclusive, in slot order
  bool fused = false;       // per-chromosome tables built inside k_scan_w (parity-alternating replicas)
  bool sliced = false;      // per-chromosome tables by k_bg_slice without its tail; k_scan_w combines
                            // the leaf sums (parity-alternating inner sums)
  bool cnt = false;         // counts plan (no position / variant_type filter): k_prep writes no per-SNP bins,
                            // the scan kernels classify the counts themselves (12 B/SNP per pass instead of 20)
  bool fst = false;         // SFS2D_F_FST: Fst per slot into d_fst
  double* d_fst = nullptr;      // where runs write Fst: d_fst_own, or the caller's (sfs2d_plan_set_fst_out)
  double* d_fst_own = nullptr;
  unsigned long long* d_fsum = nullptr;   // k_prep's per-slot Fst sums (int64 fixed point), cleared by the scan
  int hr = 1;               // k_prep LDS histogram copies per word
  uint64_t runs = 0;        // completed runs (the replica parity of a fused plan)
  int G = 64;               // 64: k_scan_w; 256: large grids (k_scan_gw when gw, else k_scan_g)
  bool gw = false;
  uint32_t* d_gscr = nullptr;   // k_scan_gw: nscr u32 histograms (nb2 words) + nscr lock words, for exact re-evaluations
  int nscr = 0;
  bool p16 = true;
  size_t scan_lds = 0, bg_lds = 0, extra_lds = 0;
  int64_t nslots = 0, nrec = 0, extra_rec = -1;
  uint32_t last_chrom = 0;
  std::vector<Tile> tiles;
  std::vector<Chunk> chunks;
  std::vector<int4> slices;
  Tile* d_tiles = nullptr;
  Chunk* d_chunks = nullptr;
  uint2* d_slots = nullptr;
  uint32_t* d_repl = nullptr;
  uint32_t* d_bcount = nullptr;   // per-chromosome inner 2D sums (k_prep -> k_bg_slice)
  uint32_t* d_done = nullptr;     // per-background completion counters of k_bg_slice
  uint32_t* d_ctr = nullptr;      // k_scan_w window pool counters, 2 parities x nchrom x CTR_POOLS lines
  double* d_bgval = nullptr;
  PL* d_tab = nullptr;
  double* d_lp = nullptr;         // log proportions alone (k_scan_w stages them in LDS)
  BgHead* d_head = nullptr;
  Bg1D* d_bg1d = nullptr;
  double* d_leafsum = nullptr;
  int2* d_leaves = nullptr;
  int4* d_nodes = nullptr;
  int4* d_slices = nullptr;
  int nleaves = 0, nnodes = 0, nlevels = 0;
  uint32_t* d_bins = nullptr;     // packed per-SNP bins written by k_prep, read by the scan kernels
  sfs2d_window* d_out = nullptr;
  uint32_t* d_err = nullptr;
  sfs2d_window* last_out = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // live timing ring: events around each kernel of every run while timing is on
  bool timing = false;
  std::vector<hipEvent_t> tev;   // 6 per sampled run (start / end of k_prep, k_bg_slice, the scan)
  int tcount = 0;
  int tmax = 0;                  // samples of the current timing session (<= tev.size() / 6)
  int tevery = 1;                // sample every tevery-th run
  int tmask = 7;                 // kernels with events: bit 0 k_prep, 1 k_bg_slice, 2 the scan kernel
  int64_t tseen = 0;             // runs since timing was set
  hipEvent_t* tpend = nullptr;   // a sampled run's events between its phase 1 and phase 2
  // events of the run being enqueued: k_prep start/stop, scan start/stop (null: not sampled).  They
  // go into the kernels' own dispatch packets (hipExtLaunchKernelGGL), so they stamp the kernel's
  // start and end as the command processor sees them -- the durations rocprofv3 reports.
  hipEvent_t kev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // multi-resolution (sfs2d_plan_attach): an attached plan shares its base's k_prep pass (bins,
  // background replicas, inner sums); the base's run scans every attached plan before its own
  std::vector<unsigned long long> slot_base_h;   // window slots per chromosome (prefix sums)
  uint32_t* d_slot_base = nullptr;
  sfs2d_plan* base = nullptr;
  std::vector<sfs2d_plan*> attached;
  uint32_t fst_m = 0;             // attached Fst: base windows per window (their sums add)
  bool fst_win = false;           // Fst by window kernels (fst_windows) instead of k_prep's sums
  bool fst_scan = false;          // Fst summed by k_scan_w itself (counts plans, small grids): k_prep has no Fst work
  bool fst_mask = true;           // Fst in the scan: the data set has SNPs with < 2 called alleles (k_scan_w FST 3 / 5)
  bool gate = false;              // Fst in the scan, folded, called counts within (n1, n2): k_scan_w's GATE variants
  bool lean = false;              // gate, fixed-bp slot records, n1p, n2p <= 31: k_scan_w's LEAN variants (same results)
  bool tri = false;               // lean, n1 = n2, the workgroup within SCAN_WT_LDS: k_scan_wt (same results)
  int sb = 8, r1 = R1;            // k_scan_w(t): windows per batched finish, lane copies of the 1D window histograms
  int nfst = 0;                   // k_bg_slice's extra Fst workgroups
  // bootstrap null (sfs2d_plan_null_run): the last call's task table and records (a read before any call: 0 records)
  std::vector<NullTask> ntask_h;
  DevBuf<NullTask> ntask;
  CallOut<sfs2d_window, 0> null_out;
  // template arguments of the scan kernel the last run launched (sfs2d_plan_scan_variant), written by
  // launch_scan from the selection it launches: {P16, FUSED, FST, CNT, GATE, TRI}, -1 where the kernel has none
  int variant[6] = {-1, -1, -1, -1, -1, -1};
  bool variant_set = false;
  // the other post-scan calls ("post-scan calls: the common skeleton"): the last call's selection on the
  // host and the device, scratch arrays, and the call's result
  CallOut<sfs2d_diversity> div_out;      // sfs2d_plan_diversity: records
  std::vector<SpecSel> spec_sel_h;       // sfs2d_plan_spectra
  DevBuf<SpecSel> spec_sel;
  CallOut<int64_t> spec_out;             // ... int64 words
  std::vector<ProjSel> proj_sel_h;       // sfs2d_plan_project
  DevBuf<ProjSel> proj_sel;
  CallOut<int64_t> proj_out;             // ... groups; its words are proj_out.n * proj_roww
  int64_t proj_roww = 0;                 // row words of the last call
  int proj_e = 0;                        // its fixed point 2^-e
  std::vector<ProjSel> pscan_sel_h;      // sfs2d_plan_project_scan: the background chromosomes' selection,
  DevBuf<ProjSel> pscan_sel;
  DevBuf<unsigned long long> pscan_bg;   // their rows
  DevBuf<double> pscan_lp;               // and ln tables
  CallOut<sfs2d_projstat> pscan_out;     // records
  // sfs2d_plan_project_null: the pools and the backgrounds' ln tables of (pnull_done, pnull_m1, pnull_m2) -- built
  // by the first call after a run or with another projection, kept for the calls that follow --, the last call's
  // selection, records and thin-slot counts
  uint64_t pnull_done = 0;               // the executed run the pool was built from (0: none)
  int32_t pnull_m1 = 0, pnull_m2 = 0;
  PnullDims pnull_dims{0, 0};
  DevBuf<uint32_t> pnull_pool;           // pool_idx: the SNPs sorted by stratum cell, stable (unused SNPs last)
  DevBuf<uint2> pnull_tab;               // (start, size) per cell
  std::vector<ProjSel> pnull_bgsel_h;    // the background chromosomes' selection,
  DevBuf<ProjSel> pnull_bgsel;
  DevBuf<unsigned long long> pnull_bg;   // their rows
  DevBuf<double> pnull_lp;               // and ln tables
  std::vector<uint32_t> pnull_sel_h;     // the entries' record indices
  DevBuf<uint32_t> pnull_sel;
  CallOut<sfs2d_projstat> pnull_out;     // records, entries x replicates
  CallOut<uint32_t> pnull_thin;          // thin slots per entry
  int64_t maxsnp = 0;                    // plan_create's bound on the SNPs of one record (Fst's e, P16)
  // runs enqueued for EXECUTION, apart from `runs` (the parity of the buffers the next enqueued run takes): a run
  // enqueued into a graph capture counts when the graph is launched (sfs2d_graph_launch), not at the capture.  The
  // "last run" of sfs2d_plan_read and the post-scan calls is the last of these; 0: the plan has no records yet.
  uint64_t done = 0;
  uint64_t null_tab_runs = ~0ull;        // fused / sliced plans: the executed run (`done`) whose tables of EVERY
                                         // chromosome are in d_tab / d_lp / d_head (their scans keep all but one
                                         // chromosome's in LDS)
};

namespace {

int set_err(sfs2d_ctx* ctx, int code, const std::string& m) {
  if (ctx) {   // (callers may use several ctx objects from several threads)
    std::lock_guard<std::mutex> g(ctx->err_mu);
    ctx->err = m;
  }
  return code;
}

#define HIPCHK(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return set_err((ctx), SFS2D_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
  } while (0)

template <typename T>
int dalloc(sfs2d_ctx* ctx, T** p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void**)p, count * sizeof(T));
  if (e != hipSuccess) return set_err(ctx, SFS2D_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  return 0;
}

void plan_free(sfs2d_plan* p) {
  if (p->base) {   // shared with the base plan
    p->d_bins = nullptr;
    p->d_repl = nullptr;
    p->d_bcount = nullptr;
    if (p->sliced) {
      p->d_tab = nullptr; p->d_lp = nullptr; p->d_head = nullptr; p->d_leafsum = nullptr; p->d_bg1d = nullptr;
    } else if (p->do_bg && p->G != WAVE) {
      p->d_tab = nullptr; p->d_lp = nullptr; p->d_head = nullptr;
    }
  }
  hipFree(p->d_slot_base); hipFree(p->d_reg);
  hipFree(p->d_tiles); hipFree(p->d_chunks); hipFree(p->d_slots); hipFree(p->d_repl); hipFree(p->d_bcount); hipFree(p->d_ctr);
  hipFree(p->d_done); hipFree(p->d_bgval); hipFree(p->d_tab); hipFree(p->d_lp); hipFree(p->d_head);
  hipFree(p->d_bg1d); hipFree(p->d_leafsum); hipFree(p->d_leaves); hipFree(p->d_nodes); hipFree(p->d_slices);
  hipFree(p->d_out); hipFree(p->d_err); hipFree(p->d_bins); hipFree(p->d_fst_own); hipFree(p->d_fsum); hipFree(p->d_gscr);
  hipFree(p->ntask.p); hipFree(p->null_out.own.p); hipFree(p->div_out.own.p);
  hipFree(p->spec_sel.p); hipFree(p->spec_out.own.p);
  hipFree(p->proj_sel.p); hipFree(p->proj_out.own.p);
  hipFree(p->pscan_sel.p); hipFree(p->pscan_bg.p); hipFree(p->pscan_lp.p); hipFree(p->pscan_out.own.p);
  hipFree(p->pnull_pool.p); hipFree(p->pnull_tab.p); hipFree(p->pnull_bgsel.p); hipFree(p->pnull_bg.p); hipFree(p->pnull_lp.p);
  hipFree(p->pnull_sel.p); hipFree(p->pnull_out.own.p); hipFree(p->pnull_thin.own.p);
  for (auto& e : p->ev) if (e) hipEventDestroy(e);
  for (auto& e : p->tev) if (e) hipEventDestroy(e);
}

// replica parity of the current run (an attached plan reads its base's k_prep output)
int plan_par(const sfs2d_plan* pl) {
  return (pl->fused || pl->sliced) ? (int)((pl->base ? pl->base->runs : pl->runs) & 1) : 0;
}
// replica parity: only fused plans alternate replicas (k_bg_slice clears what it reads)
int repl_par(const sfs2d_plan* pl) { return pl->fused ? plan_par(pl) : 0; }

// the records of the plan's last executed run: where that run wrote them (the caller's buffer or the plan's own)
const sfs2d_window* last_records(const sfs2d_plan* pl) { return pl->last_out ? pl->last_out : pl->d_out; }

// what the scan kernels stream per SNP: the bins k_prep wrote, or (counts plans) the counts themselves
const uint32_t* scan_src(const sfs2d_plan* pl) { return pl->cnt ? pl->data->counts : pl->d_bins; }

// -------------------------------------------------------------------------- kernel variants
// Each templated kernel family has one struct of its template arguments (a selection), which names the
// family's legal instantiations (legal) and numbers them (index / at); one table, variants<S>, holds the
// kernel of every legal selection at its index and null elsewhere.  Launches, occupancy and static-LDS
// queries and the dynamic-LDS limits all take their kernels from it, and one function per family
// (scan_w_sel, ..., prep_sel) is the only place that turns plan flags into template arguments.  The
// selections are made at launch (plan_attach rewrites fst_win after plan_create): a few branches and an
// indexed load.

// k_prep sums Fst per window slot (fixed point, d_fsum) and the scan takes the sums: Fst is asked for, and
// neither window kernels (fst_win) nor the scan itself (fst_scan) compute it
bool prep_sums_fst(const sfs2d_plan* pl) { return pl->fst && !pl->fst_win && !pl->fst_scan; }

// sliding and regions plans: windows that may overlap, so k_prep does not segment for them (nor sum Fst per
// window); their slot kernel runs after k_prep and their Fst is the scan's or k_fst_win's
bool free_slots(const sfs2d_plan* pl) { return pl->step > 0 || pl->regions; }

struct ScanW {   // k_scan_w<P16, FUSED, FST, CNT, GATE, LEAN>
  bool p16, fused;
  int fst;   // 0 none, 1 k_prep's sums, 2 summed in the scan, 3 the same with SNPs of < 2 called alleles dropped
  bool cnt, gate, lean;
  using Fn = void (*)(SCAN_W_ARGS);
  static constexpr int N = 128;
  constexpr int index() const { return p16 | fused << 1 | fst << 2 | cnt << 4 | gate << 5 | lean << 6; }
  static constexpr ScanW at(int i) { return {bool(i & 1), bool(i & 2), (i >> 2) & 3, bool(i & 16), bool(i & 32), bool(i & 64)}; }
  // Fst in the scan is a counts plan's; GATE and LEAN (a gated variant) are built for it alone
  constexpr bool legal() const { return fst < 2 ? !gate && !lean : cnt && (gate || !lean); }
  template <int I> static constexpr Fn kernel() { constexpr ScanW s = at(I); return k_scan_w<s.p16, s.fused, s.fst, s.cnt, s.gate, s.lean>; }
};

struct ScanWT {   // k_scan_wt<P16, FUSED, FMASK, SBN, R1N>: the lean variants on a triangle-packed window histogram
  bool p16, fused, fmask, sb32, r8;   // batches of 32 windows instead of 8; 8 lane copies of the 1D histograms instead of 4
  using Fn = void (*)(SCAN_W_ARGS);
  static constexpr int N = 32;
  constexpr int index() const { return p16 | fused << 1 | fmask << 2 | sb32 << 3 | r8 << 4; }
  static constexpr ScanWT at(int i) { return {bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8), bool(i & 16)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr ScanWT s = at(I); return k_scan_wt<s.p16, s.fused, s.fmask, s.sb32 ? 32 : 8, s.r8 ? 8 : R1>; }
};

struct ScanGW {   // k_scan_gw<P16, FST, CNT, TRI>
  bool p16, fst, cnt, tri;
  using Fn = void (*)(SCAN_W_ARGS);
  static constexpr int N = 16;
  constexpr int index() const { return p16 | fst << 1 | cnt << 2 | tri << 3; }
  static constexpr ScanGW at(int i) { return {bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8)}; }
  constexpr bool legal() const { return cnt || !tri; }   // the triangle is a counts plan's
  template <int I> static constexpr Fn kernel() { constexpr ScanGW s = at(I); return k_scan_gw<s.p16, s.fst, s.cnt, s.tri>; }
};

struct ScanG {   // k_scan_g<P16, FST, CNT>
  bool p16, fst, cnt;
  using Fn = decltype(&k_scan_g<true, true, true>);
  static constexpr int N = 8;
  constexpr int index() const { return p16 | fst << 1 | cnt << 2; }
  static constexpr ScanG at(int i) { return {bool(i & 1), bool(i & 2), bool(i & 4)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr ScanG s = at(I); return k_scan_g<s.p16, s.fst, s.cnt>; }
};

struct ScanExtra {   // k_scan_extra<P16, CNT>
  bool p16, cnt;
  using Fn = decltype(&k_scan_extra<true, true>);
  static constexpr int N = 4;
  constexpr int index() const { return p16 | cnt << 1; }
  static constexpr ScanExtra at(int i) { return {bool(i & 1), bool(i & 2)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr ScanExtra s = at(I); return k_scan_extra<s.p16, s.cnt>; }
};

struct Prep {   // k_prep<DO_BG, DO_SEG, LDS_HIST, DO_BINS, FILT, FST, JNT>
  bool bg, seg, lds, bins, filt, fst, jnt;
  using Fn = decltype(&k_prep<true, true, true, true, false, false>);
  static constexpr int N = 128;
  constexpr int index() const { return bg | seg << 1 | lds << 2 | bins << 3 | filt << 4 | fst << 5 | jnt << 6; }
  static constexpr Prep at(int i) { return {bool(i & 1), bool(i & 2), bool(i & 4), bool(i & 8), bool(i & 16), bool(i & 32), bool(i & 64)}; }
  constexpr bool legal() const {
    if (lds && !bg) return false;   // the LDS histogram is the background's
    if (jnt && !(lds && !bins && !filt && !fst)) return false;   // the joint histogram: a pass that only histograms and segments
    // a pass without bins is a counts plan's, which has no filter, or sfs2d_bg_hist's, which only histograms
    if (!bins && filt && !(bg && !seg && !fst)) return false;
    return bg || seg || bins || fst;   // (a pass with nothing to do is not launched: prep_runs)
  }
  template <int I> static constexpr Fn kernel() { constexpr Prep s = at(I); return k_prep<s.bg, s.seg, s.lds, s.bins, s.filt, s.fst, s.jnt>; }
};

struct SpecWin {   // k_spec_win<CNT, LDSH>
  bool cnt, ldsh;
  using Fn = decltype(&k_spec_win<true, true>);
  static constexpr int N = 4;
  constexpr int index() const { return cnt | ldsh << 1; }
  static constexpr SpecWin at(int i) { return {bool(i & 1), bool(i & 2)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr SpecWin s = at(I); return k_spec_win<s.cnt, s.ldsh>; }
};

struct ProjWin {   // k_proj_win<CNT, LDSH>
  bool cnt, ldsh;
  using Fn = decltype(&k_proj_win<true, true>);
  static constexpr int N = 4;
  constexpr int index() const { return cnt | ldsh << 1; }
  static constexpr ProjWin at(int i) { return {bool(i & 1), bool(i & 2)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr ProjWin s = at(I); return k_proj_win<s.cnt, s.ldsh>; }
};

struct ProjScan {   // k_proj_scan<CNT>
  bool cnt;
  using Fn = decltype(&k_proj_scan<true>);
  static constexpr int N = 2;
  constexpr int index() const { return cnt; }
  static constexpr ProjScan at(int i) { return {bool(i & 1)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr ProjScan s = at(I); return k_proj_scan<s.cnt>; }
};

struct ProjNull {   // k_proj_null<CNT>
  bool cnt;
  using Fn = decltype(&k_proj_null<true>);
  static constexpr int N = 2;
  constexpr int index() const { return cnt; }
  static constexpr ProjNull at(int i) { return {bool(i & 1)}; }
  constexpr bool legal() const { return true; }
  template <int I> static constexpr Fn kernel() { constexpr ProjNull s = at(I); return k_proj_null<s.cnt>; }
};

// entry I of family S's table: its kernel, instantiated only where the selection is legal
template <class S, int I>
constexpr typename S::Fn variant_at() {
  if constexpr (S::at(I).legal()) return S::template kernel<I>();
  else return nullptr;
}
template <class S, int... I>
constexpr std::array<typename S::Fn, sizeof...(I)> variant_table(std::integer_sequence<int, I...>) {
  return {{variant_at<S, I>()...}};
}
template <class S>
constexpr std::array<typename S::Fn, S::N> variants = variant_table<S>(std::make_integer_sequence<int, S::N>{});

// the kernel of a selection, null with SFS2D_E_ARG in *rc when it is outside its family's table
template <class S>
typename S::Fn variant(sfs2d_ctx* ctx, S s, const char* family, int* rc) {
  const typename S::Fn k = variants<S>[s.index()];
  *rc = k ? 0 : set_err(ctx, SFS2D_E_ARG, std::string(family) + ": the plan selects an instantiation outside the kernel table");
  return k;
}

// the dynamic-LDS limit on every instantiation of a family (the first error, if any): grant_lds alone calls it
template <class S>
hipError_t set_max_lds(size_t lds) {
  hipError_t e = hipSuccess;
  for (const typename S::Fn k : variants<S>) {
    if (!k) continue;
    const hipError_t ek = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = ek;
  }
  return e;
}

// The one place that raises a family's dynamic-LDS limit.  hipFuncSetAttribute sets the limit to exactly the size
// asked for, on the device's copy of a kernel and for every plan that launches it, so the limit is kept per device
// and family and only grows: a call that needs less than an earlier one leaves it alone.  Returns whether the
// family may launch with `lds` bytes of dynamic LDS (a refusal clears the HIP error: the callers fall back or
// refuse in their own words).
std::mutex lds_mu;
template <class S>
bool grant_lds(sfs2d_ctx* ctx, size_t lds) {
  static std::map<int, size_t> granted;   // device -> the dynamic LDS the family's instantiations may take
  std::lock_guard<std::mutex> lk(lds_mu);
  size_t& have = granted[ctx->device];
  if (lds <= have) return true;
  if (set_max_lds<S>(lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  have = lds;
  return true;
}

// a selection's static LDS (fallback: the query failed) and its resident workgroups per CU (0: it failed)
template <class S>
size_t static_lds(S s, size_t fallback) {
  hipFuncAttributes fa{};
  return hipFuncGetAttributes(&fa, (const void*)variants<S>[s.index()]) == hipSuccess ? fa.sharedSizeBytes : fallback;
}
template <class S>
int occupancy(S s, int block, size_t lds) {
  int occ = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, variants<S>[s.index()], block, lds) == hipSuccess ? occ : 0;
}

ScanW scan_w_sel(const sfs2d_plan* pl) {
  const bool in_scan = pl->cnt && pl->fst_scan;
  const int fst = in_scan ? (pl->fst_mask ? 3 : 2) : prep_sums_fst(pl) ? 1 : 0;
  // (gate: no SNP's key can leave the inner grid, the variants without the range test; lean: gated, and the
  // window loop's tail specialised for fixed-bp slots and n1p, n2p <= 31)
  return {pl->p16, pl->fused, fst, pl->cnt, in_scan && (pl->gate || pl->lean), in_scan && pl->lean};
}
// (tri plans are lean ones: counts, Fst in the scan, gated)
ScanWT scan_wt_sel(const sfs2d_plan* pl) { return {pl->p16, pl->fused, pl->fst_mask, pl->sb == 32, pl->r1 == 8}; }
// (large grids: Fst from k_prep's sums, taken by the scan -- unless window kernels wrote it, fst_win)
ScanGW scan_gw_sel(const sfs2d_plan* pl) { return {pl->p16, prep_sums_fst(pl), pl->cnt, pl->cnt && pl->K.ntri}; }
ScanG scan_g_sel(const sfs2d_plan* pl) { return {pl->p16, prep_sums_fst(pl), pl->cnt}; }
ScanExtra scan_extra_sel(const sfs2d_plan* pl) { return {pl->p16, pl->cnt}; }

// The scan grid is one dispatch wave of resident workgroups, sized by the occupancy of a stand-in for the
// variant that runs: Fst in the scan asked as FST 2, everything else as FST 1, and always as a counts plan.
// Every k_scan_w / k_scan_gw variant is in one VGPR bucket under amdgpu_waves_per_eu(4), but the Fst-free
// variants hold 512 B less static LDS, so a plan without Fst whose dynamic LDS lies within 512 B of the
// boundary between one and two workgroups per CU would get another grid from its own variant.  Asking about
// the variant itself is a change of behaviour, to be made with a measurement.
ScanW occ_standin(ScanW s) { s.fst = s.fst >= 2 ? 2 : 1; s.cnt = true; return s; }
ScanGW occ_standin(ScanGW s) { s.fst = s.cnt = true; return s; }

// the instantiations whose static LDS plan_create counts: the small-grid path's fit test, Fst in the scan,
// and k_prep's LDS histogram with and without its Fst sums
constexpr ScanW SCAN_W_FIT = {true, true, 1, true, false, false};
constexpr ScanW scan_w_fst_fit(bool p16) { return {p16, true, 2, true, false, false}; }
constexpr Prep prep_lds_fit(bool fst) { return {true, true, true, true, false, fst, false}; }

// k_scan_wt's workgroup, static and dynamic LDS together, at most: half a CU's 160 KB
constexpr size_t SCAN_WT_LDS = 80 * 1024;
// ... and the fewest windows per resident wavefront for which plan_create takes it
constexpr double SCAN_WT_MIN_WPW = 8.0;

// template arguments of the scan kernel being launched: {P16, FUSED, FST, CNT, GATE, TRI}, -1 where it has none
void set_variant(sfs2d_plan* pl, int p16, int fused, int fst, int cnt, int gate, int tri) {
  const int v[6] = {p16, fused, fst, cnt, gate, tri};
  std::copy(v, v + 6, pl->variant);
  pl->variant_set = true;
}

int launch_scan(sfs2d_plan* pl, sfs2d_window* out) {
  const int per_chrom = pl->prm.bg_mode == SFS2D_BG_PER_CHROM ? 1 : 0;
  const int bp = pl->prm.window_mode == SFS2D_WINDOW_BP ? 1 : 0;
  const dim3 grid((unsigned)pl->chunks.size());
  int rc = 0;
  if (pl->gw) {
    const ScanGW s = scan_gw_sel(pl);
    const ScanGW::Fn k = variant(pl->ctx, s, "k_scan_gw", &rc);
    if (!k) return rc;
    set_variant(pl, s.p16, -1, s.fst, s.cnt, -1, s.tri);
    hipExtLaunchKernelGGL(k, grid, dim3(WAVE), pl->scan_lds,
                       CTX_STREAM(pl->ctx), pl->kev[4], pl->kev[5], 0, pl->K, scan_src(pl), pl->d_chunks, pl->d_slots, pl->d_tab, pl->d_lp, pl->d_head,
                       per_chrom, pl->ctx->d_lnx, pl->ctx->d_df, out, pl->d_err, bp, pl->d_repl, pl->d_bcount,
                       0, pl->d_leaves, pl->nleaves, pl->d_nodes, pl->nnodes, pl->nlevels, -1, pl->d_fsum, pl->d_fst,
                       pl->d_ctr, (int)(pl->runs & 1), pl->d_leafsum, pl->d_bg1d, 0, pl->d_gscr, pl->nscr);
  } else if (pl->G == WAVE) {
    const ScanW s = scan_w_sel(pl);
    // (tri: the lean selection's k_scan_wt, reported as the lean variant it equals; sfs2d_plan_scan_packing tells)
    const ScanW::Fn k = pl->tri ? variant(pl->ctx, scan_wt_sel(pl), "k_scan_wt", &rc) : variant(pl->ctx, s, "k_scan_w", &rc);
    if (!k) return rc;
    set_variant(pl, s.p16, s.fused, s.fst, s.cnt, s.gate, -1);   // (LEAN: a gated variant, gate = 1)
    hipExtLaunchKernelGGL(k, grid, dim3(SBLOCK), pl->scan_lds,
                       CTX_STREAM(pl->ctx), pl->kev[4], pl->kev[5], 0, pl->K, scan_src(pl), pl->d_chunks, pl->d_slots, pl->d_tab, pl->d_lp, pl->d_head,
                       per_chrom, pl->ctx->d_lnx, pl->ctx->d_df, out, pl->d_err, bp, pl->d_repl, pl->d_bcount,
                       plan_par(pl), pl->d_leaves, pl->nleaves, pl->d_nodes, pl->nnodes, pl->nlevels,
                       pl->extra_rec >= 0 ? (int)pl->last_chrom : -1, pl->d_fsum, pl->d_fst, pl->d_ctr,
                       (int)(pl->runs & 1), pl->d_leafsum, pl->d_bg1d, pl->sliced ? 1 : 0, nullptr, 0);
  } else {
    const ScanG s = scan_g_sel(pl);
    const ScanG::Fn k = variant(pl->ctx, s, "k_scan_g", &rc);
    if (!k) return rc;
    set_variant(pl, s.p16, -1, s.fst, s.cnt, -1, -1);
    hipExtLaunchKernelGGL(k, grid, dim3(BLOCK), pl->scan_lds,
                       CTX_STREAM(pl->ctx), pl->kev[4], pl->kev[5], 0, pl->K, scan_src(pl), pl->d_chunks, pl->d_slots, pl->d_tab, pl->d_head, per_chrom,
                       pl->ctx->d_lnx, out, bp, pl->d_fsum, pl->d_fst);
  }
  HIPCHK(pl->ctx, hipGetLastError());
  return 0;
}

// whether a plan run launches k_prep at all: a counts plan's pass stores no bins, and is skipped when it has
// nothing to do (supplied background, no segmentation of its own, no Fst sums)
bool prep_runs(const sfs2d_plan* pl) {
  return !pl->tiles.empty() && (!pl->cnt || pl->do_bg || pl->do_seg || prep_sums_fst(pl));
}

// bins: a plan's pass; else the histogram-only pass of sfs2d_bg_hist
Prep prep_sel(const sfs2d_plan* pl, bool bins) {
  Prep s{};
  s.bg = !bins || pl->do_bg;
  s.seg = bins && pl->do_seg;
  s.lds = s.bg && pl->lds_hist;
  s.bins = bins && !pl->cnt;
  s.filt = pl->K.ann_want >= 0 || pl->K.has_start || pl->K.has_end;
  s.fst = bins && prep_sums_fst(pl);   // Fst sums with a plan's pass; not in sfs2d_bg_hist
  // the joint-histogram variant (plan_create sets K.jnt, with hr = 1)
  s.jnt = s.lds && !s.bins && !s.filt && !s.fst && pl->K.jnt && pl->hr == 1;
  return s;
}

int launch_prep(sfs2d_plan* pl, bool bins) {
  if (bins ? !prep_runs(pl) : pl->tiles.empty()) return 0;
  const sfs2d_data* d = pl->data;
  const Prep s = prep_sel(pl, bins);
  int rc = 0;
  const Prep::Fn k = variant(pl->ctx, s, "k_prep", &rc);
  if (!k) return rc;
  hipExtLaunchKernelGGL(k, dim3((unsigned)pl->tiles.size()), dim3(BLOCK1),
                     s.lds ? pl->bg_lds : 0, CTX_STREAM(pl->ctx), pl->kev[0], pl->kev[1], 0, pl->K, d->counts, d->pos, d->ann, pl->d_tiles,
                     pl->d_repl + (size_t)repl_par(pl) * REPL * pl->K.nchrom * pl->K.nh, pl->d_slots, pl->d_bins,
                     pl->d_bcount + (size_t)plan_par(pl) * pl->K.nchrom, pl->d_err, s.lds ? pl->hr : 1,
                     reinterpret_cast<const double2*>(pl->ctx->d_df + 2 * LNT), pl->d_fsum);
  HIPCHK(pl->ctx, hipGetLastError());
  return 0;
}

// whether a run takes its slot table from the generator's window offsets or a binary search on the
// positions instead of k_prep (seg_synth / seg_search; k_prep's Fst sums or an attached plan's use of its
// pass keep k_prep)
bool slots_only(const sfs2d_plan* pl) {
  return (pl->seg_synth || pl->seg_search) && pl->attached.empty() && !prep_sums_fst(pl);
}

hipError_t launch_slots_only(sfs2d_plan* pl) {
  const unsigned long long nw = (unsigned long long)pl->nslots;
  // (the k_prep timing slot: this is the run's segmentation stage)
  if (nw && pl->seg_synth)
    hipExtLaunchKernelGGL(k_slots_synth, dim3((unsigned)std::min<unsigned long long>(8192, (nw + 255) / 256)), dim3(256),
                          0, CTX_STREAM(pl->ctx), pl->kev[0], pl->kev[1], 0, pl->data->d_win_off, nw, pl->d_slots);
  else if (nw)
    hipExtLaunchKernelGGL(k_slots_search, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, CTX_STREAM(pl->ctx),
                          pl->kev[0], pl->kev[1], 0, pl->data->pos, pl->data->d_chrom_off, pl->d_slot_base,
                          pl->data->nchrom, (uint32_t)pl->prm.window, (uint32_t)nw, pl->d_slots);
  return hipGetLastError();
}

// a seg_index plan's slot table, ahead of its k_prep.  The two kernels are the run's segmentation +
// background stage: the stage's start event goes into this kernel's packet, its end event stays for
// k_prep's (which then carries no start event)
hipError_t launch_slots_index(sfs2d_plan* pl) {
  const uint32_t ns = (uint32_t)pl->nslots;
  if (!ns) return hipSuccess;
  const sfs2d_data* d = pl->data;
  hipExtLaunchKernelGGL(k_slots_index, dim3((ns + 255u) / 256u), dim3(256), 0, CTX_STREAM(pl->ctx), pl->kev[0], nullptr, 0,
                        d->pos, d->d_chrom_off, pl->d_slot_base, d->d_pidx, d->d_pidx_base, d->d_pidx_sh, d->nchrom,
                        (uint32_t)pl->prm.window, ns, pl->d_slots);
  pl->kev[0] = nullptr;
  return hipGetLastError();
}

// a seg_index plan's slot table for the run being enqueued.  slots_once plans: k_slots_index in the plan's first
// run alone -- afterwards the stage is k_prep alone, whose packet then carries the stage's start event as well,
// and a pass has one launch and one ~14 us chain of dependent loads less (config 3).  The plan's later runs
// come after its first in stream order, or in an order the caller makes, as its per-run state asks anyway.
// Under stream capture the kernel is launched as ever and nothing is marked: a captured launch writes nothing
// before a replay.
hipError_t stage_slots(sfs2d_plan* pl) {
  if (!pl->slots_once) return launch_slots_index(pl);
  if (pl->slots_written) return hipSuccess;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(CTX_STREAM(pl->ctx), &cs) != hipSuccess) {   // (e.g. the null stream while another stream captures)
    (void)hipGetLastError();
    return launch_slots_index(pl);
  }
  const hipError_t e = launch_slots_index(pl);
  if (e == hipSuccess && cs == hipStreamCaptureStatusNone) pl->slots_written = true;
  return e;
}

// a sliding or regions plan's slot table (after k_prep, which does not segment for it).  ev: with the k_prep
// timing events, when the run launches no k_prep (this is then its segmentation stage, as launch_slots_only)
hipError_t launch_slots_slide(sfs2d_plan* pl, bool ev) {
  const uint32_t ns = (uint32_t)pl->nslots;
  if (!ns) return hipSuccess;
  if (pl->regions)
    hipExtLaunchKernelGGL(k_slots_regions, dim3((ns + 255u) / 256u), dim3(256), 0, CTX_STREAM(pl->ctx), ev ? pl->kev[0] : nullptr,
                          ev ? pl->kev[1] : nullptr, 0, pl->data->pos, pl->data->d_chrom_off, pl->d_slot_base, pl->data->nchrom,
                          pl->d_reg, ns, pl->d_slots);
  else
    hipExtLaunchKernelGGL(k_slots_slide, dim3((ns + 255u) / 256u), dim3(256), 0, CTX_STREAM(pl->ctx), ev ? pl->kev[0] : nullptr,
                          ev ? pl->kev[1] : nullptr, 0, pl->data->pos, pl->data->d_chrom_off, pl->d_slot_base, pl->data->nchrom,
                          (uint32_t)pl->prm.window, (uint32_t)pl->step, ns, pl->d_slots);
  return hipGetLastError();
}

// Fst per slot by k_fst_win (a wavefront per window over the slot table), before the scan: sliding plans
// whose scan does not sum Fst itself, attached plans of sliced bases
hipError_t launch_fst_win(sfs2d_plan* a) {
  const uint32_t ns = (uint32_t)a->nslots;
  if (!ns) return hipSuccess;
  const dim3 gf((unsigned)std::min<uint32_t>(2048u, (ns + 3u) / 4u));
  if (a->cnt)
    hipLaunchKernelGGL(k_fst_win<true>, gf, dim3(256), 0, CTX_STREAM(a->ctx), a->K, a->data->counts, scan_src(a), a->d_slots,
                       reinterpret_cast<const double2*>(a->ctx->d_df + 2 * LNT), a->d_fst, ns);
  else
    hipLaunchKernelGGL(k_fst_win<false>, gf, dim3(256), 0, CTX_STREAM(a->ctx), a->K, a->data->counts, scan_src(a), a->d_slots,
                       reinterpret_cast<const double2*>(a->ctx->d_df + 2 * LNT), a->d_fst, ns);
  return hipGetLastError();
}

// per-run per-chromosome backgrounds
hipError_t launch_bg_slices(sfs2d_plan* pl) {
  hipExtLaunchKernelGGL(k_bg_slice, dim3((unsigned)pl->slices.size() + 1 + (unsigned)pl->nfst, (unsigned)pl->nbg), dim3(KBLOCK), 0,
                     CTX_STREAM(pl->ctx), pl->kev[2], pl->kev[3], 0, pl->K, pl->d_repl, pl->d_bcount + (size_t)plan_par(pl) * pl->K.nchrom, pl->d_tab,
                     pl->d_lp, pl->d_head, pl->d_leafsum, pl->d_bg1d, pl->d_done, pl->d_slices, (int)pl->slices.size(),
                     pl->d_leaves, pl->nleaves, pl->d_nodes, pl->nnodes, pl->nlevels, pl->sliced ? 0 : 1, pl->nfst,
                     pl->data->counts, scan_src(pl), pl->d_slots, reinterpret_cast<const double2*>(pl->ctx->d_df + 2 * LNT),
                     pl->d_fst, (uint32_t)pl->nslots);
  return hipGetLastError();
}

// one supplied background (values uploaded to d_bgval)
hipError_t launch_finalize(sfs2d_plan* pl, int integer_values) {
  const size_t lds = pl->K.nt <= FIN_LDS_BINS ? sizeof(double) * pl->K.nt : 0;
  hipLaunchKernelGGL(k_bg_finalize, dim3(1), dim3(FBLOCK), lds, CTX_STREAM(pl->ctx), pl->K, integer_values, pl->d_bgval,
                     pl->d_bgval, pl->d_tab, pl->d_lp, pl->d_head, pl->d_leaves, pl->nleaves, pl->d_nodes, pl->nnodes);
  return hipGetLastError();
}

int launch_scan_any(sfs2d_plan* pl, sfs2d_window* out) {
  int rc = pl->chunks.empty() ? 0 : launch_scan(pl, out);
  if (rc || pl->extra_rec < 0) return rc;
  const sfs2d_data* d = pl->data;
  const ScanExtra::Fn k = variant(pl->ctx, scan_extra_sel(pl), "k_scan_extra", &rc);
  if (!k) return rc;
  hipLaunchKernelGGL(k, dim3(1), dim3(WAVE), pl->extra_lds, CTX_STREAM(pl->ctx), pl->K, scan_src(pl),
                     d->pos, pl->last_chrom, d->d_chrom_off, pl->d_tab, pl->d_head,
                     pl->prm.bg_mode == SFS2D_BG_PER_CHROM ? 1 : 0, pl->ctx->d_lnx, out, (long long)pl->extra_rec);
  HIPCHK(pl->ctx, hipGetLastError());
  return 0;
}

// one attached plan inside its base's run: its window slots (fixed bp: binary search on the
// positions), its Fst sums (from the base's), then its scan against the base's k_prep output
int launch_attached(sfs2d_plan* a) {
  const sfs2d_data* d = a->data;
  const uint32_t ns = (uint32_t)a->nslots;
  if (!ns) { a->runs++; a->done += a->ctx->capturing ? 0 : 1; return 0; }
  const dim3 g((ns + 255) / 256);
  if (a->regions)
    hipLaunchKernelGGL(k_slots_regions, g, dim3(256), 0, CTX_STREAM(a->ctx), d->pos, d->d_chrom_off, a->d_slot_base,
                       d->nchrom, a->d_reg, ns, a->d_slots);
  else if (a->step)
    hipLaunchKernelGGL(k_slots_slide, g, dim3(256), 0, CTX_STREAM(a->ctx), d->pos, d->d_chrom_off, a->d_slot_base,
                       d->nchrom, (uint32_t)a->prm.window, (uint32_t)a->step, ns, a->d_slots);
  else if (a->prm.window_mode == SFS2D_WINDOW_BP)
    hipLaunchKernelGGL(k_slots_bp, g, dim3(256), 0, CTX_STREAM(a->ctx), d->pos, d->d_chrom_off, a->d_slot_base,
                       d->nchrom, (uint32_t)a->prm.window, ns, a->d_slots);
  if (a->fst_m)
    hipLaunchKernelGGL(k_fst_agg, g, dim3(256), 0, CTX_STREAM(a->ctx), a->base->d_fsum, a->base->d_slot_base,
                       a->d_slot_base, d->nchrom, a->fst_m, ns,
                       std::max(0, a->base->K.fst_e - a->K.fst_e), a->d_fsum);
  if (a->fst_win) launch_fst_win(a);   // before the scan clears the slots
  const int rc = launch_scan_any(a, a->d_out);
  a->last_out = a->d_out;
  a->runs++;
  if (!a->ctx->capturing) a->done++;
  return rc;
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI

extern "C" {

// an ablation build (-DSFS2D_ABL=..., timing only, wrong results) reports a negative version, which the
// loaders refuse (sfs2d/_lib.py) unless SFS2D_ALLOW_ABLATION=1 is set by the timing tool
int sfs2d_abi_version(void) { return SFS2D_ABL ? -SFS2D_ABL : SFS2D_ABI_VERSION; }

const char* sfs2d_last_error(const sfs2d_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int sfs2d_ctx_create(int device, sfs2d_ctx** out) {
  if (!out) return SFS2D_E_ARG;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return SFS2D_E_HIP;
  if (device < 0 || device >= ndev) return SFS2D_E_ARG;
  sfs2d_ctx* c = new sfs2d_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return SFS2D_E_HIP;
  }
  c->stream = c->own;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->ncu = prop.multiProcessorCount;
  if (dalloc(c, &c->d_lnx, LNX_N) || dalloc(c, &c->d_df, 2 * LNT + 2 * RCPN) || dalloc(c, &c->d_hw, RCPN)) {
    hipFree(c->d_lnx); hipFree(c->d_df); hipStreamDestroy(c->own); delete c; return SFS2D_E_NOMEM;
  }
  {   // 1 / h(n): the harmonic sums in ascending order of i (sfs2d/diversity.py forms the same doubles)
    std::vector<double> hw(RCPN, 0.0);
    double h = 0.0;
    for (int n = 2; n < RCPN; ++n) {
      h += 1.0 / (double)(n - 1);
      hw[n] = 1.0 / h;
    }
    if (hipMemcpy(c->d_hw, hw.data(), sizeof(double) * RCPN, hipMemcpyHostToDevice) != hipSuccess) {
      hipFree(c->d_lnx); hipFree(c->d_df); hipFree(c->d_hw); hipStreamDestroy(c->own); delete c; return SFS2D_E_HIP;
    }
  }
  hipLaunchKernelGGL(k_init_lnx, dim3(LNX_N / 256), dim3(256), 0, c->stream, c->d_lnx, c->d_df, c->d_df + LNT,
                     c->d_df + 2 * LNT);
  if (hipStreamSynchronize(c->stream) != hipSuccess) {
    hipFree(c->d_lnx); hipFree(c->d_df); hipFree(c->d_hw); hipStreamDestroy(c->own); delete c; return SFS2D_E_HIP;
  }
  *out = c;
  return 0;
}

int sfs2d_ctx_destroy(sfs2d_ctx* ctx) {
  if (!ctx) return SFS2D_E_ARG;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(CTX_STREAM(ctx));
  hipFree(ctx->d_lnx);
  hipFree(ctx->d_df);
  hipFree(ctx->d_hw);
  hipFree(ctx->d_lf);
  if (ctx->stagger) hipEventDestroy(ctx->stagger);
  hipStreamDestroy(ctx->own);
  delete ctx;
  return 0;
}

// NULL is the HIP null stream (ordered with the process's blocking streams), not the ctx's own: a
// caller passing its default stream's handle (torch's is 0) gets the ordering it expects
int sfs2d_ctx_set_stream(sfs2d_ctx* ctx, void* stream) {
  if (!ctx) return SFS2D_E_ARG;
  ctx->stream = (hipStream_t)stream;
  return 0;
}

int sfs2d_ctx_get_stream(const sfs2d_ctx* ctx, void** stream) {
  if (!ctx || !stream) return SFS2D_E_ARG;
  *stream = (void*)ctx->stream;
  return 0;
}

int sfs2d_ctx_use_own_stream(sfs2d_ctx* ctx) {
  if (!ctx) return SFS2D_E_ARG;
  ctx->stream = ctx->own;
  return 0;
}

static int data_meta(sfs2d_ctx* ctx, sfs2d_data* d, const int64_t* chrom_off, int32_t nchrom, int64_t n) {
  if (nchrom < 0 || n < 0 || n > 0xfffffff0ll) return set_err(ctx, SFS2D_E_ARG, "bad n / nchrom");
  if (nchrom > 0 && !chrom_off) return set_err(ctx, SFS2D_E_ARG, "chrom_off is NULL");
  d->chrom_off.assign(chrom_off, chrom_off + nchrom + 1);
  if (nchrom == 0) d->chrom_off.assign(1, 0);
  if (d->chrom_off.front() != 0 || d->chrom_off.back() != n) return set_err(ctx, SFS2D_E_ARG, "chrom_off must span [0, n]");
  for (int c = 0; c < nchrom; ++c)
    if (d->chrom_off[c + 1] < d->chrom_off[c]) return set_err(ctx, SFS2D_E_ARG, "chrom_off not monotone");
  d->n = n;
  d->nchrom = nchrom;
  if (dalloc(ctx, &d->d_chrom_off, (size_t)nchrom + 1)) return SFS2D_E_NOMEM;
  HIPCHK(ctx, hipMemcpy(d->d_chrom_off, d->chrom_off.data(), sizeof(long long) * (nchrom + 1), hipMemcpyHostToDevice));
  return 0;
}

int sfs2d_data_upload(sfs2d_ctx* ctx, const uint32_t* counts, const uint32_t* pos, const uint16_t* ann_id, int64_t n,
                      const int64_t* chrom_off, int32_t nchrom, sfs2d_data** out) {
  if (!ctx || !out || (n > 0 && (!counts || !pos))) return set_err(ctx, SFS2D_E_ARG, "null argument");
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  sfs2d_data* d = new sfs2d_data();
  d->ctx = ctx;
  d->owned = true;
  int rc = data_meta(ctx, d, chrom_off, nchrom, n);
  // padded: the kernels issue aligned 16-B loads that may run up to 15 bytes past element n-1
  const size_t npad = ((size_t)n + 3) / 4 * 4 + 64;
  if (!rc) rc = dalloc(ctx, &d->counts, npad);
  if (!rc) rc = dalloc(ctx, &d->pos, npad);
  if (!rc) rc = dalloc(ctx, &d->ann, npad);
  if (!rc && (hipMemset(d->counts, 0, npad * 4) != hipSuccess || hipMemset(d->pos, 0, npad * 4) != hipSuccess))
    rc = set_err(ctx, SFS2D_E_HIP, "hipMemset");
  if (rc) { hipFree(d->counts); hipFree(d->pos); hipFree(d->ann); hipFree(d->d_chrom_off); delete d; return rc; }
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpy(d->counts, counts, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d->pos, pos, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      if (ann_id) e = hipMemcpy(d->ann, ann_id, sizeof(uint16_t) * n, hipMemcpyHostToDevice);
      else e = hipMemset(d->ann, 0, sizeof(uint16_t) * n);
    }
  }
  if (e != hipSuccess) {
    hipFree(d->counts); hipFree(d->pos); hipFree(d->ann); hipFree(d->d_chrom_off); delete d;
    return set_err(ctx, SFS2D_E_HIP, std::string("upload: ") + hipGetErrorString(e));
  }
  d->last_pos.assign(nchrom, 0);
  d->host_pos.assign(pos, pos + n);
  {
    uint32_t m1 = 0, m2 = 0;
    bool low = false;
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t c = counts[i];
      const uint32_t n1c = (c & 0xffu) + ((c >> 8) & 0xffu), n2c = ((c >> 16) & 0xffu) + (c >> 24);
      m1 = std::max(m1, n1c);
      m2 = std::max(m2, n2c);
      low |= std::min(n1c, n2c) < 2u;
    }
    d->max_nc1 = m1;
    d->max_nc2 = m2;
    d->low_nc = low;
  }
  for (int c = 0; c < nchrom; ++c) {
    int64_t s = d->chrom_off[c], t = d->chrom_off[c + 1];
    if (t > s) d->last_pos[c] = pos[t - 1];
    for (int64_t i = s + 1; i < t; ++i)
      if (pos[i] <= pos[i - 1]) { d->strict = false; break; }
  }
  *out = d;
  return 0;
}

int sfs2d_data_wrap_device(sfs2d_ctx* ctx, const uint32_t* d_counts, const uint32_t* d_pos, const uint16_t* d_ann_id,
                           int64_t n, const int64_t* chrom_off, const uint32_t* chrom_last_pos, int32_t nchrom,
                           sfs2d_data** out) {
  if (!ctx || !out || (n > 0 && (!d_counts || !d_pos)) || (nchrom > 0 && !chrom_last_pos))
    return set_err(ctx, SFS2D_E_ARG, "null argument");
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  sfs2d_data* d = new sfs2d_data();
  d->ctx = ctx;
  d->owned = false;
  int rc = data_meta(ctx, d, chrom_off, nchrom, n);
  if (rc) { hipFree(d->d_chrom_off); delete d; return rc; }
  if (((uintptr_t)d_counts & 15) || ((uintptr_t)d_pos & 15) || ((uintptr_t)d_ann_id & 7)) {
    hipFree(d->d_chrom_off); delete d;
    return set_err(ctx, SFS2D_E_ARG, "device arrays must be 16-byte aligned (and readable to round_up(n, 4))");
  }
  d->counts = const_cast<uint32_t*>(d_counts);
  d->pos = const_cast<uint32_t*>(d_pos);
  if (d_ann_id) {
    d->ann = const_cast<uint16_t*>(d_ann_id);
  } else {
    const size_t na = ((size_t)n + 3) / 4 * 4 + 64;
    if (dalloc(ctx, &d->ann, na) || hipMemset(d->ann, 0, sizeof(uint16_t) * na) != hipSuccess) {
      hipFree(d->d_chrom_off); delete d; return SFS2D_E_NOMEM;
    }
    d->ann_owned = true;
  }
  d->last_pos.assign(chrom_last_pos, chrom_last_pos + nchrom);
  d->strict = true;   // contract: positions strictly increasing within each chromosome
  if (n > 0) {   // the largest called counts (see max_nc1), one pass over the caller's counts
    uint32_t* d_m = nullptr;
    uint32_t hm[3] = {0, 0, 0};
    hipError_t e = hipMalloc((void**)&d_m, 3 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(d_m, 0, 3 * sizeof(uint32_t), CTX_STREAM(ctx));
    if (e == hipSuccess) {
      const unsigned grid = (unsigned)std::min<int64_t>(4096, (n + 1023) / 1024);
      hipLaunchKernelGGL(k_max_called, dim3(grid), dim3(256), 0, CTX_STREAM(ctx), d->counts, (unsigned long long)n, d_m);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hm, d_m, sizeof(hm), hipMemcpyDeviceToHost, CTX_STREAM(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(CTX_STREAM(ctx));
    hipFree(d_m);
    if (e != hipSuccess) {
      if (d->ann_owned) hipFree(d->ann);
      hipFree(d->d_chrom_off); delete d;
      return set_err(ctx, SFS2D_E_HIP, std::string("wrap_device: ") + hipGetErrorString(e));
    }
    d->max_nc1 = hm[0];
    d->max_nc2 = hm[1];
    d->low_nc = hm[2] != 0u;
  } else {
    d->max_nc1 = d->max_nc2 = 0;
    d->low_nc = false;
  }
  *out = d;
  return 0;
}

int sfs2d_data_synth_sims(sfs2d_ctx* ctx, const sfs2d_synth_params* sp, const uint16_t* win_snps,
                          const uint32_t* miss_cdf1, int32_t nm1, const uint32_t* miss_cdf2, int32_t nm2,
                          sfs2d_data** out) {
  if (!ctx || !sp || !out || !miss_cdf1 || !miss_cdf2 || nm1 < 1 || nm2 < 1 ||
      (sp->n_replicates && sp->n_windows && !win_snps))
    return set_err(ctx, SFS2D_E_ARG, "null argument");
  if (sp->n1p < 1 || sp->n2p < 1 || 2 * sp->n1p > 255 || 2 * sp->n2p > 255 || sp->window_bp < 1 ||
      (unsigned long long)sp->n_windows * sp->window_bp > 0xffffffffull)
    return set_err(ctx, SFS2D_E_ARG, "bad synthetic parameters");
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t nw = (uint64_t)sp->n_replicates * sp->n_windows;
  std::vector<unsigned long long> woff(nw + 1, 0);
  std::vector<int64_t> coff(sp->n_replicates + 1, 0);
  for (uint64_t w = 0; w < nw; ++w) {
    if (win_snps[w] > sp->window_bp) return set_err(ctx, SFS2D_E_ARG, "more SNPs than bp in a window");
    woff[w + 1] = woff[w] + win_snps[w];
  }
  for (uint32_t r = 0; r < sp->n_replicates; ++r) coff[r + 1] = (int64_t)woff[(uint64_t)(r + 1) * sp->n_windows];
  const int64_t n = (int64_t)woff[nw];
  sfs2d_data* d = new sfs2d_data();
  d->ctx = ctx;
  d->owned = true;
  int rc = data_meta(ctx, d, coff.data(), (int32_t)sp->n_replicates, n);
  if (rc) { hipFree(d->d_chrom_off); delete d; return rc; }
  const size_t np = ((size_t)n + 3) / 4 * 4 + 64;   // readable to round_up(n, 4) (+ k_scan_w overhang)
  unsigned long long* d_woff = nullptr;
  uint32_t* d_mt = nullptr;
  if (dalloc(ctx, &d->counts, np) || dalloc(ctx, &d->pos, np) || dalloc(ctx, &d->ann, np) ||
      dalloc(ctx, &d_woff, nw + 1) || dalloc(ctx, &d_mt, (size_t)nm1 + nm2)) {
    hipFree(d->counts); hipFree(d->pos); hipFree(d->ann); hipFree(d_woff); hipFree(d->d_chrom_off); delete d;
    return SFS2D_E_NOMEM;
  }
  hipError_t e = hipMemsetAsync(d->ann, 0, sizeof(uint16_t) * np, CTX_STREAM(ctx));
  if (e == hipSuccess) e = hipMemsetAsync(d->counts, 0, sizeof(uint32_t) * np, CTX_STREAM(ctx));
  if (e == hipSuccess) e = hipMemsetAsync(d->pos, 0, sizeof(uint32_t) * np, CTX_STREAM(ctx));
  if (e == hipSuccess) e = hipMemcpyAsync(d_woff, woff.data(), sizeof(unsigned long long) * (nw + 1), hipMemcpyHostToDevice, CTX_STREAM(ctx));
  if (e == hipSuccess) e = hipMemcpyAsync(d_mt, miss_cdf1, sizeof(uint32_t) * nm1, hipMemcpyHostToDevice, CTX_STREAM(ctx));
  if (e == hipSuccess) e = hipMemcpyAsync(d_mt + nm1, miss_cdf2, sizeof(uint32_t) * nm2, hipMemcpyHostToDevice, CTX_STREAM(ctx));
  if (e == hipSuccess && nw) {
    SynthP S;
    S.seed = sp->seed; S.gen = sp->generation; S.nwin = sp->n_windows; S.ws = sp->window_bp;
    S.n1 = 2u * (uint32_t)sp->n1p; S.n2 = 2u * (uint32_t)sp->n2p; S.nm1 = (uint32_t)nm1; S.nm2 = (uint32_t)nm2;
    const unsigned grid = (unsigned)std::min<uint64_t>(16384, (nw + 3) / 4);
    hipLaunchKernelGGL(k_synth_sims, dim3(grid), dim3(256), 0, CTX_STREAM(ctx), S, d_woff, (unsigned long long)nw,
                       d_mt, d_mt + nm1, d->counts, d->pos);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(CTX_STREAM(ctx));
  hipFree(d_mt);
  if (e != hipSuccess) {
    hipFree(d_woff);
    hipFree(d->counts); hipFree(d->pos); hipFree(d->ann); hipFree(d->d_chrom_off); delete d;
    return set_err(ctx, SFS2D_E_HIP, std::string("synthetic data: ") + hipGetErrorString(e));
  }
  d->d_win_off = d_woff;   // the window offsets stay: fixed-bp plans of window_bp read their slots from them
  d->win_bp = sp->window_bp;
  d->win_per_chrom = sp->n_windows;
  d->last_pos.assign(sp->n_replicates, sp->n_windows * sp->window_bp);   // upper bound: trailing slots stay empty
  d->strict = true;
  d->max_nc1 = 2u * (uint32_t)sp->n1p;   // k_synth_sims: ref + alt + missing = 2 pop_size
  d->max_nc2 = 2u * (uint32_t)sp->n2p;
  *out = d;
  return 0;
}

int sfs2d_data_read(const sfs2d_data* d, uint32_t* counts, uint32_t* pos, int64_t n) {
  if (!d || n != d->n) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = d->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  if (counts && n) HIPCHK(ctx, hipMemcpy(counts, d->counts, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (pos && n) HIPCHK(ctx, hipMemcpy(pos, d->pos, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

int sfs2d_data_free(sfs2d_data* d) {
  if (!d) return SFS2D_E_ARG;
  hipSetDevice(d->ctx->device);
  if (d->owned) { hipFree(d->counts); hipFree(d->pos); }
  if (d->owned || d->ann_owned) hipFree(d->ann);
  hipFree(d->d_chrom_off);
  hipFree(d->d_win_off);
  hipFree(d->d_pidx); hipFree(d->d_pidx_base); hipFree(d->d_pidx_sh);
  delete d;
  return 0;
}

// The data set's position index (k_pos_index), built on first use: 0.1 ms for 5e7 SNPs, <= 0.25 B/SNP plus
// two words per chromosome.  A chromosome without SNPs has no entries.
static int data_pos_index(sfs2d_ctx* ctx, const sfs2d_data* d) {
  std::lock_guard<std::mutex> g(d->pidx_mu);
  if (d->d_pidx) return 0;
  const int nc = d->nchrom;
  std::vector<uint32_t> base(nc + 1, 0), sh(std::max(1, nc), 0);
  unsigned long long nent = 0;
  for (int c = 0; c < nc; ++c) {
    const int64_t len = d->chrom_off[c + 1] - d->chrom_off[c];
    if (len > 0) {
      const unsigned long long want = (unsigned long long)std::max<int64_t>(1, len / 16);
      uint32_t s = 0;
      while (((unsigned long long)d->last_pos[c] >> s) + 1ull > want) ++s;   // (s <= 32: one cell)
      sh[c] = s;
      nent += ((unsigned long long)d->last_pos[c] >> s) + 2ull;
    }
    base[c + 1] = (uint32_t)nent;
  }
  if (nent > 0xffffffffull) return set_err(ctx, SFS2D_E_ARG, "position index too large");
  uint32_t *idx = nullptr, *db = nullptr, *ds = nullptr;
  int rc = dalloc(ctx, &idx, (size_t)nent);
  rc = rc ? rc : dalloc(ctx, &db, base.size());
  rc = rc ? rc : dalloc(ctx, &ds, sh.size());
  hipError_t e = hipSuccess;
  if (!rc) {
    hipStream_t st = CTX_STREAM(ctx);
    e = hipMemcpyAsync(db, base.data(), sizeof(uint32_t) * base.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ds, sh.data(), sizeof(uint32_t) * sh.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && nent) {
      hipLaunchKernelGGL(k_pos_index, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, st, d->pos, d->d_chrom_off, db, ds,
                         nc, (uint32_t)nent, idx);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // (base and sh leave scope)
  }
  if (rc || e != hipSuccess) {
    hipFree(idx); hipFree(db); hipFree(ds);
    return rc ? rc : set_err(ctx, SFS2D_E_HIP, std::string("position index: ") + hipGetErrorString(e));
  }
  d->d_pidx = idx; d->d_pidx_base = db; d->d_pidx_sh = ds;
  return 0;
}

static int make_kparams(sfs2d_ctx* ctx, const sfs2d_params* prm, int nchrom, KParams* K) {
  *K = KParams{};   // (every field defined: e.g. ntri stays 0 unless a plan takes k_scan_gw's triangle)
  if (!prm) return set_err(ctx, SFS2D_E_ARG, "params is NULL");
  if (prm->n1p < 1 || prm->n2p < 1 || 2 * prm->n1p > 255 || 2 * prm->n2p > 255)
    return set_err(ctx, SFS2D_E_ARG, "pop sizes must satisfy 1 <= pop_size and 2*pop_size <= 255 (u8 counts)");
  if (prm->window_mode != SFS2D_WINDOW_BP && prm->window_mode != SFS2D_WINDOW_SNPS)
    return set_err(ctx, SFS2D_E_ARG, "bad window_mode");
  if (prm->window < 1 || prm->window > 0xffffffffll) return set_err(ctx, SFS2D_E_ARG, "window must be in [1, 2^32)");
  if (prm->bg_mode != SFS2D_BG_PER_CHROM && prm->bg_mode != SFS2D_BG_SUPPLIED) return set_err(ctx, SFS2D_E_ARG, "bad bg_mode");
  K->n1p = prm->n1p; K->n2p = prm->n2p; K->n1 = 2 * prm->n1p; K->n2 = 2 * prm->n2p;
  K->nb2 = (K->n1 + 1) * (K->n2 + 1);
  K->h1a = K->nb2; K->h1b = K->nb2 + K->n1 + 1; K->nh = (K->h1b + K->n2 + 1 + 3) & ~3;   // 16-B rows
  K->t1a = K->nb2; K->t1b = K->nb2 + K->n1p + 1; K->nt = K->t1b + K->n2p + 1;
  K->rtn = wl_rtn(K->n1p, K->n2p);   // (plans: widened to the data's largest called count)
  K->fold = prm->fold ? 1 : 0;
  K->fold_thr = prm->fold ? K->n1p + K->n2p : 0x7fffffff;
  K->ann_want = prm->ann_want;
  K->has_start = prm->has_start ? 1 : 0; K->has_end = prm->has_end ? 1 : 0;
  K->start_pos = prm->start_pos; K->end_pos = prm->end_pos;
  K->ws = (unsigned)prm->window;
  div_magic(K->ws, &K->wmag, &K->wsh1, &K->wsh2);
  K->nchrom = nchrom;
  K->fst_e = 40;   // plan_create narrows this to the plan's windows
  K->fst_scale = std::ldexp(1.0, K->fst_e);
  return 0;
}

// plan_create's environment knobs, read once per plan (null: not set); each is parsed where it applies
struct Knobs {
  const char* seg = std::getenv("SFS2D_SEG");                // prep / search / index: where fixed-bp slots come from
  const char* lnl = std::getenv("SFS2D_LNL");                // 0: k_scan_gw without its LDS ln table
  const char* gw = std::getenv("SFS2D_GW");                  // 0 / 1: large grids by k_scan_g / k_scan_gw
  const char* fused = std::getenv("SFS2D_FUSED");            // 0 / 1: small-grid tables sliced / fused
  const char* fst_scan = std::getenv("SFS2D_FST_SCAN");      // 0: Fst from k_prep's sums, not summed in the scan
  const char* lean = std::getenv("SFS2D_LEAN");              // 0: the gated variants where the lean ones apply
  const char* tri = std::getenv("SFS2D_TRI");                // 0: the lean variants where the triangle-packed ones apply; 1: packed below SCAN_WT_MIN_WPW too
  const char* sb = std::getenv("SFS2D_SB");                  // A/B: 8 / 32 windows per batched finish of a tri plan
  const char* r1 = std::getenv("SFS2D_R1");                  // A/B: 4 / 8 lane copies of a tri plan's 1D window histograms
  const char* slots_once = std::getenv("SFS2D_SLOTS_ONCE");  // 0: index plans write their slot table every run
  const char* wgs = std::getenv("SFS2D_WGS");                // tuning: scan workgroups in all
  const char* gwwin = std::getenv("SFS2D_GWWIN");            // tuning: k_scan_gw windows per workgroup of a small chromosome
  const char* pools = std::getenv("SFS2D_POOLS");            // tuning: most window pools per chromosome
  const char* tile = std::getenv("SFS2D_TILE");              // tuning: SNPs per k_prep tile
  const char* jnt = std::getenv("SFS2D_JNT");                // 0 / 1: k_prep's joint histogram never / whatever the tile size
};

// a regions plan's intervals (host arrays, grouped by chromosome; checked by check_regions)
struct RegionList {
  const int32_t* chrom;
  const uint32_t *first, *last;
  int64_t n;
};

static int plan_create(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int force_sliced, int64_t step,
                       const RegionList* rg, sfs2d_plan** out);

int sfs2d_plan_create(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, sfs2d_plan** out) {
  return plan_create(ctx, data, prm, -1, 0, nullptr, out);
}

// a sliding plan's step against its params (after make_kparams accepted them)
static int check_step(sfs2d_ctx* ctx, const sfs2d_params* prm, int64_t step) {
  if (prm->window_mode != SFS2D_WINDOW_BP) return set_err(ctx, SFS2D_E_ARG, "sliding windows need fixed-bp windows (SFS2D_WINDOW_BP)");
  if (step < 1 || step > prm->window) return set_err(ctx, SFS2D_E_ARG, "step must be in [1, window]");
  if (prm->window % step != 0) return set_err(ctx, SFS2D_E_ARG, "step must divide the window");
  if (prm->window / step > 64) return set_err(ctx, SFS2D_E_ARG, "window / step must be <= 64");
  if (prm->flags & SFS2D_F_PREV_EXTRA)
    return set_err(ctx, SFS2D_E_ARG, "SFS2D_F_PREV_EXTRA (quirk Q9 of the disjoint window loop) is not defined for sliding windows");
  return 0;
}

int sfs2d_plan_create_sliding(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int64_t step,
                              sfs2d_plan** out) {
  if (!ctx || !data || !prm || !out) return set_err(ctx, SFS2D_E_ARG, "null argument");
  *out = nullptr;
  KParams K;
  int rc = make_kparams(ctx, prm, data->nchrom, &K);
  if (!rc) rc = check_step(ctx, prm, step);
  // step == window is the disjoint geometry: the ordinary plan itself (records and Fst byte-equal by construction)
  return rc ? rc : plan_create(ctx, data, prm, -1, step == prm->window ? 0 : step, nullptr, out);
}

// a regions plan's params and list (after make_kparams accepted the params); *longest: the longest region in bp,
// what the plan's copy of params->window holds (2^32 - 1 for the one length above it, first = 0 .. last = 2^32 - 1)
static int check_regions(sfs2d_ctx* ctx, const sfs2d_params* prm, int nchrom, const RegionList& rg, int64_t* longest) {
  if (prm->window_mode != SFS2D_WINDOW_BP) return set_err(ctx, SFS2D_E_ARG, "regions are intervals in bp (SFS2D_WINDOW_BP), not SNP-count windows");
  if (prm->flags & SFS2D_F_PREV_EXTRA)
    return set_err(ctx, SFS2D_E_ARG, "SFS2D_F_PREV_EXTRA (quirk Q9 of the disjoint window loop) is not defined for regions");
  if (!rg.chrom || !rg.first || !rg.last) return set_err(ctx, SFS2D_E_ARG, "regions: null array");
  if (rg.n < 1) return set_err(ctx, SFS2D_E_ARG, "regions: the list must hold at least one region");
  if (rg.n >= 0x80000000ll) return set_err(ctx, SFS2D_E_ARG, "regions: the list must hold fewer than 2^31 regions");
  int64_t lg = 1;
  for (int64_t i = 0; i < rg.n; ++i) {
    if (rg.chrom[i] < 0 || rg.chrom[i] >= nchrom)
      return set_err(ctx, SFS2D_E_ARG, "regions: chrom out of range at region " + std::to_string(i));
    if (i && rg.chrom[i] < rg.chrom[i - 1])
      return set_err(ctx, SFS2D_E_ARG, "regions: chrom decreases at region " + std::to_string(i) + " (group the list by chromosome)");
    if (rg.first[i] > rg.last[i]) return set_err(ctx, SFS2D_E_ARG, "regions: first > last at region " + std::to_string(i));
    lg = std::max<int64_t>(lg, (int64_t)rg.last[i] - (int64_t)rg.first[i] + 1);
  }
  *longest = std::min<int64_t>(lg, 0xffffffffll);
  return 0;
}

// Regions: the windows are a caller's list of intervals (include/sfs2d.h).  The plan is built as a sliding plan is
// (k_prep without segmentation, a slot kernel of its own after it, Fst by the scan or k_fst_win), with the list
// as its slot table's source.
int sfs2d_plan_create_regions(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, const int32_t* chrom,
                              const uint32_t* first, const uint32_t* last, int64_t n, sfs2d_plan** out) {
  if (!ctx || !data || !prm || !out) return set_err(ctx, SFS2D_E_ARG, "null argument");
  *out = nullptr;
  KParams K;
  int rc = make_kparams(ctx, prm, data->nchrom, &K);
  const RegionList rg{chrom, first, last, n};
  sfs2d_params p = *prm;
  if (!rc) rc = check_regions(ctx, prm, data->nchrom, rg, &p.window);
  return rc ? rc : plan_create(ctx, data, &p, -1, 0, &rg, out);
}

// force_sliced: -1 choose (windows per wave), 0 fused, 1 sliced (attached plans follow their base)
// step: 0 disjoint windows; > 0 a sliding plan (checked by check_step)
// rg: null, or a regions plan's list (checked by check_regions; step 0, prm->window the longest region)
static int plan_create(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int force_sliced, int64_t step,
                       const RegionList* rg, sfs2d_plan** out) {
  if (!ctx || !data || !prm || !out) return set_err(ctx, SFS2D_E_ARG, "null argument");
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  KParams K;
  int rc = make_kparams(ctx, prm, data->nchrom, &K);
  if (rc) return rc;
  const Knobs env;
  // (slide: every rule below that holds for windows k_prep does not segment -- a regions plan follows them all)
  const bool slide = step > 0 || rg;
  const int64_t adv = step > 0 ? step : prm->window;   // bp from one window's start to the next's
  sfs2d_plan* pl = new sfs2d_plan();
  pl->ctx = ctx; pl->data = data; pl->prm = *prm; pl->K = K;
  // no SNP of the data set has more called alleles than 2 pop_size in either population (max_nc1 / max_nc2)
  const bool nc_ok = data->max_nc1 <= (uint32_t)K.n1 && data->max_nc2 <= (uint32_t)K.n2;
  pl->K.nc_ok = nc_ok ? 1 : 0;
  const bool bp = prm->window_mode == SFS2D_WINDOW_BP;
  pl->step = step > 0 ? step : 0;
  pl->regions = rg != nullptr;
  pl->do_seg = bp && !slide;   // (a sliding plan's slots: k_slots_slide after k_prep; a regions plan's: k_slots_regions)
  pl->do_bg = prm->bg_mode == SFS2D_BG_PER_CHROM;
  pl->nbg = pl->do_bg ? std::max(1, data->nchrom) : 1;
  const int nc = data->nchrom;

  // window slots + scan chunks
  std::vector<unsigned long long> slot_base(nc + 1, 0);
  uint32_t last_c = 0;
  bool any = false;
  std::vector<int64_t> rcount(rg ? nc : 0, 0);   // regions per chromosome: a chromosome's slots, SNPs or none
  if (rg)
    for (int64_t i = 0; i < rg->n; ++i) rcount[rg->chrom[i]]++;
  for (int c = 0; c < nc; ++c) {
    const int64_t len = data->chrom_off[c + 1] - data->chrom_off[c];
    int64_t ns = rg ? rcount[c] : 0;
    if (len > 0 && rg) {
      last_c = (uint32_t)c;
      any = true;
    } else if (len > 0) {
      // (sliding: slot j starts at j step + 1, the last one holds the chromosome's last SNP)
      if (bp) ns = (int64_t)(data->last_pos[c] ? (data->last_pos[c] - 1u) / (uint32_t)adv : 0u) + 1;
      else ns = len / prm->window;
      last_c = (uint32_t)c;
      any = true;
    }
    slot_base[c + 1] = slot_base[c] + ns;
  }
  pl->nslots = (int64_t)slot_base[nc];
  pl->slot_base_h = slot_base;
  // counts plan: no filter (the scan kernels classify counts without positions / annotations)
  pl->cnt = prm->ann_want < 0 && !prm->has_start && !prm->has_end;
  // a supplied background: no k_prep pass reads (and validates) the counts of a counts plan, so one is
  // taken only when no SNP can raise an error (max_nc1 / max_nc2); else the bins pipeline's k_prep
  // classifies every SNP and reports KeyError / out-of-grid keys as the reference raises them
  if (pl->cnt && prm->bg_mode != SFS2D_BG_PER_CHROM &&
      !(data->max_nc1 <= (uint32_t)K.n1 && data->max_nc2 <= (uint32_t)K.n2))
    pl->cnt = false;
  // generated replicates (sfs2d_data_synth_sims) scanned with the generator's window length: slot s of
  // replicate c is the generator's window c * win_per_chrom + w, whose SNPs it placed in that window
  // ((pos - 1) / ws == w), so the slot table is the window offsets (k_slots_synth) -- when every
  // replicate holds SNPs (the slot numbering skips empty chromosomes) and the plan has no other k_prep
  // work (a counts plan with a supplied background; see slots_only).
  // Any other fixed-bp counts plan with a supplied background (no k_prep histograms) takes its slots by
  // binary search on the resident positions (k_slots_search) instead of k_prep's segmentation pass.
  // SFS2D_SEG=prep forces k_prep's segmentation, SFS2D_SEG=search the search (never the generator's
  // offsets: what a real replicate VCF gets); both are selected by tests/test_synth_device.py.  SFS2D_SEG=index
  // names what plans with per-chromosome backgrounds take unless it is prep (seg_index below, tests/test_slot_index.py)
  const bool seg_prep = env.seg && std::strcmp(env.seg, "prep") == 0, seg_srch = env.seg && std::strcmp(env.seg, "search") == 0;
  if (bp && !slide && data->d_win_off && (uint32_t)prm->window == data->win_bp && pl->cnt && !pl->do_bg &&
      pl->nslots == (int64_t)nc * (int64_t)data->win_per_chrom) {
    bool all = true;
    for (int c = 0; c < nc && all; ++c) all = data->chrom_off[c + 1] > data->chrom_off[c];
    pl->seg_synth = all && !seg_prep && !seg_srch;
  }
  // (Not with per-chromosome backgrounds, whose k_prep runs anyway: there this search -- ~21 dependent
  // loads over ~6 lines per boundary -- before a counts-only k_prep cost more than the positions it saved
  // k_prep: config 3: k_prep 83.5 -> 64.5 us but one pass 0.214 -> 0.225 ms, the overlapped step 0.184 ->
  // 0.191 ms, config 2 2.4e8 -> 2.0e8 windows/s; as extra blocks of k_prep itself, concurrent with its
  // tiles: 0.185 -> 0.193 ms; profiles/r06e_*, r06f_*.  Those plans take their slots from the data set's
  // position index instead, seg_index below: one index read and a search inside one or two lines.)
  pl->seg_search = bp && !slide && pl->cnt && !pl->do_bg && !pl->seg_synth && !seg_prep;
  pl->K.nm1 = data->n > 0 ? (uint32_t)(data->n - 1) : 0u;
  pl->K.kmul = (uint32_t)(pl->K.n2 + 1) | (1u << 16);
  pl->K.n2inv = (uint32_t)(0x100000000ull / (uint32_t)(pl->K.n2 + 1)) + 1u;   // n2 + 1 >= 3
  pl->K.n12 = (uint32_t)pl->K.n1 | ((uint32_t)pl->K.n2 << 16);
  pl->K.lim12 = (uint32_t)(pl->K.n1p - 1) | ((uint32_t)(pl->K.n2p - 1) << 16);
  {   // Fst's reciprocals in LDS cover the data's largest called count: the reference counts SNPs whose
      // r + a exceeds 2 pop_size as long as the key stays in the grid (u8 counts: n <= 510)
    const uint32_t mx = std::min<uint32_t>(510u, std::max(data->max_nc1, data->max_nc2));
    pl->K.rtn = std::max(wl_rtn(K.n1p, K.n2p), (int)((mx + 2u) & ~1u));
  }
  if (pl->nslots > 0x7fffffffll) { delete pl; return set_err(ctx, SFS2D_E_ARG, "too many window slots (window too small)"); }
  pl->extra_rec = ((prm->flags & SFS2D_F_PREV_EXTRA) && bp && any) ? pl->nslots : -1;
  pl->nrec = pl->nslots + (pl->extra_rec >= 0 ? 1 : 0);

  // LDS strategy: a wavefront per window with u16-packed 2D bins for small grids, a workgroup per
  // window for large ones; u16 bins need < 65536 SNPs of one window in one bin.
  // (maxsnp: the most SNPs any window can hold, bounding the Fst fixed-point sums)
  int64_t maxc = 0;
  for (int c = 0; c < nc; ++c) maxc = std::max<int64_t>(maxc, data->chrom_off[c + 1] - data->chrom_off[c]);
  int64_t maxsnp = maxc;
  if (!bp || data->strict) maxsnp = std::min<int64_t>(maxc, prm->window);
  bool p16_ok;
  if (!bp) {
    p16_ok = prm->window <= 65535;
  } else if (!rg && data->strict && prm->window <= 65535) {
    p16_ok = true;   // unique positions: a window of ws bp holds at most ws SNPs
  } else if (!data->host_pos.empty() || data->n == 0) {
    // exact longest window run from the host copy of the positions
    int64_t longest = 0;
    // (regions: the SNP count of every region, by the definition k_slots_regions implements -- two searches each)
    for (int64_t i = 0; rg && i < rg->n; ++i) {
      const uint32_t* hp = data->host_pos.data();
      const uint32_t* cb = hp + data->chrom_off[rg->chrom[i]];
      const uint32_t* ce = hp + data->chrom_off[rg->chrom[i] + 1];
      const uint32_t* b = std::lower_bound(cb, ce, rg->first[i]);
      const uint32_t* e = std::upper_bound(b, ce, rg->last[i]);   // the first pos >= last + 1, without the + 1
      longest = std::max<int64_t>(longest, e - b);
    }
    for (int c = 0; c < nc && !rg; ++c) {
      int64_t run = 0;
      uint32_t pw = 0xffffffffu;
      if (slide) {   // a bound: the most SNPs in any ws bp that start at an SNP (every sliding window lies in one)
        int64_t j = data->chrom_off[c];
        for (int64_t i = data->chrom_off[c]; i < data->chrom_off[c + 1]; ++i) {
          while ((int64_t)data->host_pos[i] - (int64_t)data->host_pos[j] >= prm->window) ++j;
          longest = std::max(longest, i - j + 1);
        }
        continue;
      }
      for (int64_t i = data->chrom_off[c]; i < data->chrom_off[c + 1]; ++i) {
        const uint32_t p = data->host_pos[i];
        const uint32_t w = p ? (p - 1u) / (uint32_t)prm->window : 0u;
        run = (w == pw) ? run + 1 : 1;
        pw = w;
        longest = std::max(longest, run);
      }
    }
    p16_ok = longest <= 65535;
    maxsnp = std::min(maxsnp, longest);
  } else {
    p16_ok = false;
  }
  pl->p16 = p16_ok;
  pl->maxsnp = maxsnp;
  {
    // Fst fixed point 2^e: maxsnp terms of |x| <= 1 stay below 2^62 (e = 46 for 20 kb windows)
    int b = 0;
    while (b < 62 && (int64_t(1) << b) <= maxsnp) ++b;   // bit length of maxsnp
    pl->K.fst_e = std::max(8, std::min(FST_E_MAX, 61 - b));
    pl->K.fst_scale = std::ldexp(1.0, pl->K.fst_e);
  }
  pl->G = (K.nb2 <= 8192) ? 64 : 256;
  {
    const int core = (pl->p16 ? (K.nb2 + 1) / 2 : K.nb2) + (K.n1p + 1) + (K.n2p + 1);
    pl->extra_lds = (size_t)core * 4;
    if (pl->G == WAVE) {
      // k_scan_w: lp table (even-rounded) + D + F tables (+ Fst's reciprocals when Fst is asked for: the
      // scan may sum it), then 8 per-wave histogram blocks (also the fused prologue's scratch: u1 words,
      // 1D proportions, leaf accumulators and sums)
      const int h2w = pl->p16 ? (((K.nb2 + 1) / 2 + 3) & ~3) : ((K.nb2 + 3) & ~3);
      const int per = (h2w + R1 * (K.n1p + 1) + R1 * (K.n2p + 1) + 3) & ~3;   // (no trash words: scan_w_small)
      const size_t hist_words = std::max<size_t>((size_t)(SBLOCK / WAVE) * per, (size_t)FUSED_VCNT + K.nt + 16);
      const size_t rt = (prm->flags & SFS2D_F_FST) ? 2 * (size_t)pl->K.rtn : 0;
      pl->scan_lds = sizeof(double) * (size_t)(((K.nt + 1) & ~1) + LNT + LNF + rt) + hist_words * 4;
      // with the static LDS of the variant that uses most (the batched finish's per-wave arrays, Fst);
      // grids whose workgroup does not fit the 160 KB (e.g. 81 x 81) take the large-grid kernels
      if (pl->scan_lds + static_lds(SCAN_W_FIT, 4096) > 160 * 1024) pl->G = 256;
    }
    if (pl->G != WAVE) {
      pl->scan_lds = (size_t)(core + TRASH + 2) * 4 + 32 * 8 + 32 * 8;
      // k_scan_gw (a wavefront per window, tables from L2) when its one-wave workgroups, whose LDS
      // holds only the wave's histograms, still leave >= 2 wavefronts per CU (101 x 101: 7);
      // otherwise k_scan_g (a workgroup per window).  SFS2D_GW=0/1 forces one.
      // u8-packed 2D bins; counts plans with folded square grids keep only the reachable triangle
      // (k_scan_gw TRI: x1 + x2 <= n; 101 x 101: 5,151 of 10,201 bins -- half the LDS per wave).
      // x1 + x2 <= n holds only when every SNP's called counts r + a are <= 2 pop_size (then a folded
      // key has r1 + r2 <= 2n - (a1 + a2) < n); the reference counts any in-grid key
      // (twoDSFS_class.py:198-217), so data with a larger called count (max_nc1 / max_nc2, known at
      // upload) keep the full k2-indexed grid
      if (pl->cnt && prm->fold && K.n1 == K.n2 && data->max_nc1 <= (uint32_t)K.n1 && data->max_nc2 <= (uint32_t)K.n2)
        K.ntri = pl->K.ntri = (K.n1 + 1) * (K.n1 + 2) / 2;
      const int h2w = (((K.ntri ? K.ntri : K.nb2) + 3) / 4 + 3) & ~3;
      size_t gw_lds = (size_t)(h2w + R1GW * (K.n1p + 1) + R1GW * (K.n2p + 1) + TRASH) * 4;
      int occ = 0;
      if (gw_lds <= 160 * 1024) {
        // workgroups per CU of the plan's stand-in with lds bytes of dynamic LDS (0: more than the 160 KB, or no answer)
        const ScanGW gs = occ_standin(scan_gw_sel(pl));
        auto gw_occ = [&](size_t lds) {
          if (lds > 160 * 1024) return 0;
          if (lds > 64 * 1024) grant_lds<ScanGW>(ctx, lds);
          return occupancy(gs, WAVE, lds);
        };
        occ = gw_occ(gw_lds);
        // the LDS ln table (KParams::lnl) when it costs no workgroup per CU (config 4's 101 x 101 triangle:
        // 16 one-wave workgroups either way; config 5's 201 x 151 grid would lose one)
        const size_t lds2 = gw_lds + 8 + (size_t)LNL * 8;
        if (gw_occ(lds2) == occ && occ >= 2 && !(env.lnl && env.lnl[0] == '0')) {
          gw_lds = lds2;
          K.lnl = pl->K.lnl = 1;
        }
        (void)hipGetLastError();
        pl->gw = occ >= 2;   // measured on 201 x 151 with u16 bins (2 per CU): 22 vs 32 us for k_scan_g
        if (env.gw) pl->gw = occ >= 1 && env.gw[0] == '1';
      }
      if (pl->gw) pl->scan_lds = gw_lds;
    }
  }
  if (pl->scan_lds > 160 * 1024) {
    delete pl;
    return set_err(ctx, SFS2D_E_ARG, "2D grid too large for LDS with 32-bit bins (windows of >= 65536 SNPs)");
  }
  // per-chromosome backgrounds on the small-grid path: k_bg_slice (many workgroups per background)
  // then k_scan_w copies the table and combines the leaf sums in its prologue ("sliced"); the fused
  // alternative (every scan workgroup sums the replicas and builds the table itself) is kept for
  // comparison (SFS2D_FUSED=1): it is ~2x longer per workgroup
  // for the small-grid path.  Which wins depends on windows per wavefront: with about one window
  // each (1e6-SNP chromosome: 2.8k windows on 4k resident wavefronts) the table build IS the
  // kernel's critical path and the sliced path is ~5% faster per run; with tens of windows each
  // (config 3: 34) the fused prologue is amortised and its loop variant is faster.
  // SFS2D_FUSED=0/1 forces one.
  const bool small = pl->do_bg && pl->G == WAVE;
  const double wpw = (double)pl->nslots / (2.0 * ctx->ncu * (SBLOCK / WAVE));   // windows per resident wave
  pl->sliced = small && wpw < 4.0;
  if (env.fused) pl->sliced = small && env.fused[0] == '0';
  if (force_sliced >= 0) pl->sliced = small && force_sliced == 1;
  pl->fused = small && !pl->sliced;
  // Fst of sliced fixed-bp plans: by extra k_bg_slice workgroups (the GPU is mostly idle during
  // that latency-bound kernel) instead of k_prep's per-SNP sums (config 2: k_prep -3 us)
  pl->fst = (prm->flags & SFS2D_F_FST) != 0;
  // Fst of counts plans on the small-grid path is summed by k_scan_w over the rows it streams
  // (fst_scan): k_prep then has no Fst work and stays bandwidth-bound (config 3: 147 -> 83 us) while
  // the scan, bound by its LDS pipe and VALU issue, grows (143 -> 210 us; an LDS copy of the
  // reciprocal table: 262 us).  One pass alone is ~2% slower than with k_prep's sums, but passes
  // overlapped on streams gain (config 2, 3 streams: 14.0 -> 12.8 us per pass; config 3, 2 streams
  // capped at 1 scan workgroup per CU: 293 -> 281 us), and an attached plan can then have Fst on any
  // window (profiles/r03k_fst_scan.txt).  SFS2D_FST_SCAN=0: k_prep's fixed-point sums / k_bg_slice's
  // Fst workgroups instead (attached Fst then needs fixed-bp windows the base's divide)
  pl->fst_scan = false;
  if (pl->fst && pl->cnt && pl->G == WAVE && !pl->gw) {
    pl->fst_scan = !(env.fst_scan && env.fst_scan[0] == '0');
    // its variant's static LDS must fit beside the dynamic (a failed query: no Fst in the scan)
    if (pl->fst_scan && pl->scan_lds + static_lds(scan_w_fst_fit(pl->p16), 160 * 1024) > 160 * 1024) pl->fst_scan = false;
  }
  // folded, and every called count within 2 pop_size (the condition of k_scan_gw's triangle below): a
  // folded key has x1 <= n1, x2 <= n2 and x1 + x2 <= (n1 + n2) / 2 -- inside the grid and never the excluded
  // last bin -- so the scan's per-SNP range test on it is dead (k_scan_w's GATE variants, built for Fst in
  // the scan).  Over-called or unfolded data keep the test.
  pl->gate = pl->fst_scan && prm->fold && nc_ok;
  // gated plans whose windows come from fixed-bp slot records and whose folded 1D spectra fit one half-wave
  // each: the LEAN variants (SFS2D_LEAN=0: the gated variants, for comparison -- the results are the same)
  pl->lean = pl->gate && bp && K.n1p <= 31 && K.n2p <= 31;
  if (env.lean) pl->lean = pl->lean && env.lean[0] != '0';
  // lean plans with n1 = n2: the window histogram packed into its reachable bins (k_scan_wt), and the LDS that
  // frees spent on batches of 32 windows and 8 lane copies of the 1D histograms -- while the workgroup, static LDS
  // included, stays within SCAN_WT_LDS, so that two of them share a CU; otherwise the lean variant as it was.
  // Only for plans with at least SCAN_WT_MIN_WPW windows per resident wavefront (wpw, above): with up to 8 a
  // wavefront flushes as often in batches of 32 as in batches of 8, and the plan would pay the packed index's 16
  // VALU per row-pair block for nothing (config 2, ~0.7 windows per wavefront: +2% per pass).
  // SFS2D_TRI=0: the lean variant, for comparison (the results are the same); SFS2D_TRI=1: the packed variant
  // whatever the windows per wavefront (the tests' small genomes), still within SCAN_WT_LDS
  // (SFS2D_SB / SFS2D_R1: the arms with one ingredient less, for comparison; any other value is refused, for every
  // plan, so that a mistyped comparison does not measure the default)
  const std::string sbv = env.sb ? env.sb : "32", r1v = env.r1 ? env.r1 : "8";
  if ((sbv != "8" && sbv != "32") || (r1v != "4" && r1v != "8")) {
    delete pl;
    return set_err(ctx, SFS2D_E_ARG, "SFS2D_SB must be 8 or 32 and SFS2D_R1 4 or 8 (the instantiations k_scan_wt has)");
  }
  const bool tri_gate = wpw >= SCAN_WT_MIN_WPW || (env.tri && env.tri[0] == '1');
  if (pl->lean && K.n1 == K.n2 && !(env.tri && env.tri[0] == '0') && tri_gate) {
    const int sb = sbv == "8" ? 8 : 32, r1 = r1v == "4" ? 4 : 8;
    const int nh2 = (K.nb2 + K.n1) / 2 + 1;
    const int h2w = pl->p16 ? (((nh2 + 1) / 2 + 3) & ~3) : ((nh2 + 3) & ~3);
    const int per = (h2w + r1 * (K.n1p + 1) + r1 * (K.n2p + 1) + 3) & ~3;
    const size_t hist_words = std::max<size_t>((size_t)(SBLOCK / WAVE) * per, (size_t)FUSED_VCNT + K.nt + 16);
    const size_t lds = sizeof(double) * (size_t)(((K.nt + 1) & ~1) + LNT + LNF + 2 * (size_t)pl->K.rtn) + hist_words * 4;
    const ScanWT fit = {pl->p16, true, true, sb == 32, r1 == 8};
    if (lds + static_lds(fit, SCAN_WT_LDS) <= SCAN_WT_LDS) {
      pl->tri = true;
      pl->sb = sb;
      pl->r1 = r1;
      pl->scan_lds = lds;
    }
  }
  const PwTree pw = pw_plan(K.nb2 - 3);
  pl->fst_mask = data->low_nc;
  pl->fst_win = pl->sliced && bp && pl->fst && !pl->fst_scan;
  // a sliding plan has no k_prep sums (they are per disjoint window): Fst where the scan does not sum it is
  // k_fst_win over the sliding slots, launched on its own before the scan
  if (slide) pl->fst_win = pl->fst && !pl->fst_scan;
  // Fixed-bp counts plans with per-chromosome backgrounds whose k_prep has no per-window work (no Fst sums
  // of its own): the slot table from the data set's position index (k_slots_index, ahead of k_prep on the
  // plan's stream), and k_prep without segmentation -- it then reads no positions (4 B/SNP instead of 8)
  // and has no window-id header, neighbour load or boundary branch.  SFS2D_SEG=prep: k_prep's
  // segmentation.  (An attached plan takes its slots from k_slots_bp inside its base's run; its base qualifies.)
  // Only for positions the library owns (an upload, generated replicates): a caller's wrapped device arrays may
  // be written after the plan is created, in stream order ahead of a run (tests/test_stream_contract.py), or
  // between runs, so no index built from them once holds; they keep k_prep's segmentation.
  pl->seg_index = bp && !slide && pl->cnt && pl->do_bg && !seg_prep && force_sliced < 0 && data->owned &&
                  !prep_sums_fst(pl);
  if (pl->seg_index) {
    if ((rc = data_pos_index(ctx, data))) { delete pl; return rc; }
    pl->do_seg = false;
  }
  // ... and with Fst summed in the scan no kernel but k_slots_index stores to the table (the scan's slot clear
  // is the Fst-free variants'): it is written once per plan.  SFS2D_SLOTS_ONCE=0: every run, for comparison
  pl->slots_once = pl->seg_index && pl->fst_scan;
  if (env.slots_once) pl->slots_once = pl->slots_once && env.slots_once[0] != '0';
  pl->nfst = pl->fst_win && !slide ? (int)std::min<int64_t>(1024, std::max<int64_t>(1, (pl->nslots + 7) / 8)) : 0;   // ~1 window per wave
  if (pl->scan_lds > 64 * 1024) {   // (k_scan_gw's: with its occupancy, above)
    grant_lds<ScanW>(ctx, pl->scan_lds);
    grant_lds<ScanWT>(ctx, pl->scan_lds);
    grant_lds<ScanG>(ctx, pl->scan_lds);
  }
  if (pl->extra_lds > 64 * 1024) grant_lds<ScanExtra>(ctx, pl->extra_lds);

  // scan work items.  k_scan_w: about one workgroup per resident slot (one dispatch wave, no
  // tail), shared among the chromosomes by window count; each wavefront takes one static window,
  // then windows from its chromosome's pool counters until they run dry (windows cost up to ~3x
  // each other, so static chunks left the slowest workgroups 2x behind the median).
  // k_scan_g: two windows per workgroup.
  if (pl->G == WAVE || pl->gw) {
    // (the grid is one dispatch wave of resident workgroups: occupancy of the variant's stand-in, occ_standin)
    int occ = pl->gw ? occupancy(occ_standin(scan_gw_sel(pl)), WAVE, pl->scan_lds)
                     : pl->tri ? occupancy(scan_wt_sel(pl), SBLOCK, pl->scan_lds)
                               : occupancy(occ_standin(scan_w_sel(pl)), SBLOCK, pl->scan_lds);
    if (occ < 1) occ = 1;
    if (prm->scan_wgs_per_cu > 0 && (int)prm->scan_wgs_per_cu < occ) occ = (int)prm->scan_wgs_per_cu;
    int64_t cap = (int64_t)occ * ctx->ncu;
    if (pl->gw) pl->nscr = (int)cap;   // one exact-path histogram per resident wavefront
    if (env.wgs) cap = std::max<int64_t>(1, std::atoll(env.wgs));
    const double S = (double)std::max<unsigned long long>(1, slot_base[nc] - slot_base[0]);
    const uint32_t NW = pl->gw ? 1u : (uint32_t)(SBLOCK / WAVE);   // wavefronts per workgroup
    int64_t gw_win = 64;   // k_scan_gw: windows per workgroup of a small chromosome
    if (env.gwwin) gw_win = std::max<int64_t>(1, std::atoll(env.gwwin));
    std::vector<double> order;
    for (int c = 0; c < nc; ++c) {
      const uint32_t ns = (uint32_t)(slot_base[c + 1] - slot_base[c]);
      if (!ns) continue;
      const uint32_t wmax = (ns + NW - 1) / NW;
      int64_t want = std::llround(cap * (ns / S));
      // k_scan_gw has no table prologue: many small chromosomes (sims batches: thousands of
      // replicates) get ~64 windows per workgroup instead of one workgroup each, which would leave
      // the last dispatch wave's workgroups running alone
      if (pl->gw) want = std::max<int64_t>(want, (ns + gw_win - 1) / gw_win);
      const uint32_t nwg = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(wmax, want));
      uint32_t npool = std::min<uint32_t>(nwg, CTR_POOLS);
      if (env.pools) npool = std::max(1u, std::min<uint32_t>(npool, (uint32_t)std::atoi(env.pools)));
      for (uint32_t k = 0; k < nwg; ++k) {
        Chunk ch{};
        ch.chrom = (uint32_t)c; ch.slot_lo = (uint32_t)slot_base[c]; ch.slot_hi = (uint32_t)slot_base[c + 1];
        ch.wid_lo = 0; ch.cb = (uint32_t)data->chrom_off[c];
        ch.first = k * NW; ch.nstatic = nwg * NW; ch.pool = npool | ((k % npool) << 16);
        pl->chunks.push_back(ch);
        order.push_back((k + 0.5) / nwg);
      }
    }
    // spread every chromosome's workgroups evenly over the grid: the first ~ncu workgroups are the
    // older of the two on their CU (issue priority), so a chromosome made only of younger ones
    // finished ~25% later than one of older ones; mixed, each pool drains at the common rate
    std::vector<size_t> idx(pl->chunks.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return order[a] < order[b]; });
    std::vector<Chunk> sorted(idx.size());
    for (size_t i = 0; i < idx.size(); ++i) sorted[i] = pl->chunks[idx[i]];
    pl->chunks.swap(sorted);
  } else {
    constexpr uint32_t CH = 2;
    for (int c = 0; c < nc; ++c)
      for (unsigned long long s = slot_base[c]; s < slot_base[c + 1]; s += CH) {
        Chunk ch{};
        ch.chrom = (uint32_t)c; ch.slot_lo = (uint32_t)s;
        ch.slot_hi = (uint32_t)std::min<unsigned long long>(s + CH, slot_base[c + 1]);
        ch.wid_lo = (uint32_t)(s - slot_base[c]);
        ch.cb = (uint32_t)data->chrom_off[c];
        ch.nstatic = ch.slot_hi - ch.slot_lo; ch.pool = 1;
        pl->chunks.push_back(ch);
      }
  }
  pl->last_chrom = last_c;

  // k_prep tiles (never crossing a chromosome); k_prep always runs (it writes the per-SNP bins)
  int64_t tileT = 0;
  {
    const int64_t n = data->n;
    // ~1000+ tiles for big inputs (several workgroups per CU), >= 4096 SNPs each (flush amortised)
    // (with k_prep's Fst sums, <= 32k SNPs per tile keep a tile's windows in its LDS sums down to
    // ~128-SNP windows; every tile flushes its LDS histogram, so no smaller tiles than that otherwise)
    const int64_t Tmax = prep_sums_fst(pl) ? 32768 : 65536;
    int64_t T = std::max<int64_t>(4096, std::min<int64_t>(Tmax, (n / 768 + 4095) / 4096 * 4096));
    if (env.tile) T = std::max<int64_t>(2048, std::atoll(env.tile) & ~int64_t(3));
    tileT = T;
    // tile edges on absolute multiples of 4 SNPs (T is): only a chromosome's first and last step
    // take k_prep's masked edge path, every interior step of every tile the fast one
    for (int c = 0; c < nc; ++c)
      for (int64_t s = data->chrom_off[c]; s < data->chrom_off[c + 1];) {
        const int64_t e = std::min<int64_t>((s & ~int64_t(3)) + T, data->chrom_off[c + 1]);
        Tile t{};
        t.chrom = (uint32_t)c; t.begin = (uint32_t)s;
        t.end = (uint32_t)e;
        s = e;
        t.cb = (uint32_t)data->chrom_off[c]; t.ce = (uint32_t)data->chrom_off[c + 1];
        t.sbase = (uint32_t)slot_base[c];
        t.nslots = (uint32_t)(slot_base[c + 1] - slot_base[c]);
        pl->tiles.push_back(t);
      }
  }
  // one LDS copy per histogram word: four interleaved copies (lane & 3, fewer same-address atomics)
  // cost more in zeroing and flushing than they saved (k_prep config 2 10.3 vs 10.9 us, config 3
  // 183 vs 187 us)
  pl->hr = 1;
  pl->bg_lds = ((size_t)K.nh * pl->hr + WAVE) * 4;   // + 64 lane trash words
  {
    // the LDS histogram must fit beside the static LDS of the k_prep variant that will run: the Fst
    // variant (Fst not taken from k_bg_slice) holds ~20 KB of window sums and reciprocals, so e.g.
    // pop_size 95 / 95 (148 KB of histogram) takes the global-atomic histogram with Fst
    const bool kfst = prep_sums_fst(pl);
    const size_t stat = static_lds(prep_lds_fit(kfst), kfst ? 24 * 1024 : 1024);
    pl->lds_hist = pl->bg_lds + stat <= 160 * 1024;
    // k_prep's joint (alt1, alt2) histogram (prep_tile, JNT): counts plans whose k_prep only histograms
    // and segments, with tiles of >= 16k SNPs (its margins pass at the tile's end cost config 2's 4k-SNP
    // tiles more than the atomics saved: 2.25e8 vs 2.32-2.46e8 windows/s, profiles/r06i_prep_joint_hist.txt),
    // while the LDS stays <= 64 KB (nb2 words more).  SFS2D_JNT=0: three atomics per SNP; =1: the joint
    // histogram whatever the tile size (tests)
    const size_t jl = pl->bg_lds + (size_t)K.nb2 * 4;
    const bool jwant = env.jnt ? env.jnt[0] == '1' : tileT >= 16384;
    // (one histogram copy per word: the joint path indexes the LDS histogram unreplicated; a counts plan has
    // no filter, so its histogram pass always launches the JNT instantiation and uses these nb2 words)
    if (pl->lds_hist && pl->hr == 1 && pl->cnt && !kfst && jl + stat <= 64 * 1024 && jwant) {
      pl->K.jnt = K.nb2;
      pl->bg_lds = jl;
    }
  }
  // the large dynamic LDS refused: the global-atomic histogram instead
  if (pl->lds_hist && pl->bg_lds > 64 * 1024 && !grant_lds<Prep>(ctx, pl->bg_lds)) pl->lds_hist = false;
  hipFuncSetAttribute((const void*)k_bg_finalize, hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)(sizeof(double) * FIN_LDS_BINS));

  // numpy pairwise plan over the 2D inner bins except the last (p[:-1] of bins[1:-1]) and the
  // k_bg_slice bin ranges: LEAVES_PER_SLICE leaves each, the first from bin 0, the last to nb2
  pl->nleaves = (int)pw.leaves.size();
  pl->nnodes = (int)pw.nodes.size();
  pl->nlevels = pw.nlevels;
  if (pl->nleaves > PW_MAX_LEAVES) { delete pl; return set_err(ctx, SFS2D_E_ARG, "grid too large for the pairwise plan"); }
  const int lps = LEAVES_PER_SLICE;   // (1 / 2 / 4 leaves per slice measure the same, tools/lps_probe.sh)
  for (int j = 0; j < pl->nleaves; j += lps) {
    const int jl = std::min(pl->nleaves, j + lps);
    const int kb = j == 0 ? 0 : 1 + pw.leaves[j].x;
    const int ke = jl == pl->nleaves ? K.nb2 : 1 + pw.leaves[jl].x;
    pl->slices.push_back(make_int4(kb, ke, j, jl));
  }
  if (pl->slices.empty()) pl->slices.push_back(make_int4(0, K.nb2, 0, 0));

  hipStream_t st = CTX_STREAM(ctx);
  rc = 0;
  rc = rc ? rc : dalloc(ctx, &pl->d_tiles, pl->tiles.size());
  rc = rc ? rc : dalloc(ctx, &pl->d_chunks, pl->chunks.size());
  rc = rc ? rc : dalloc(ctx, &pl->d_slots, (size_t)pl->nslots + 1);
  const size_t nrepl = pl->do_bg ? (size_t)(pl->fused ? 2 : 1) * REPL * nc * K.nh : 1;
  rc = rc ? rc : dalloc(ctx, &pl->d_repl, nrepl);
  rc = rc ? rc : dalloc(ctx, &pl->d_bcount, (size_t)2 * std::max(1, nc));
  rc = rc ? rc : dalloc(ctx, &pl->d_done, (size_t)pl->nbg);
  const size_t nctr = (size_t)2 * std::max(1, nc) * CTR_POOLS * CTR_STRIDE;
  rc = rc ? rc : dalloc(ctx, &pl->d_ctr, nctr);
  const size_t ngscr = pl->gw ? (size_t)pl->nscr * (K.nb2 + 1) : 0;
  if (pl->gw) rc = rc ? rc : dalloc(ctx, &pl->d_gscr, ngscr);
  rc = rc ? rc : dalloc(ctx, &pl->d_bgval, (size_t)pl->nbg * K.nt);
  rc = rc ? rc : dalloc(ctx, &pl->d_tab, (size_t)pl->nbg * K.nt);
  rc = rc ? rc : dalloc(ctx, &pl->d_lp, (size_t)pl->nbg * K.nt);
  rc = rc ? rc : dalloc(ctx, &pl->d_head, (size_t)pl->nbg);
  rc = rc ? rc : dalloc(ctx, &pl->d_bg1d, (size_t)pl->nbg);
  rc = rc ? rc : dalloc(ctx, &pl->d_leafsum, (size_t)pl->nbg * std::max(1, pl->nleaves));
  rc = rc ? rc : dalloc(ctx, &pl->d_leaves, pw.leaves.size());
  rc = rc ? rc : dalloc(ctx, &pl->d_nodes, pw.nodes.size());
  rc = rc ? rc : dalloc(ctx, &pl->d_slices, pl->slices.size());
  const size_t nbins = pl->cnt ? 4 : ((size_t)data->n + 3) / 4 * 4 + SCAN_PAD;   // k_scan_w's step loads overhang n
  rc = rc ? rc : dalloc(ctx, &pl->d_bins, nbins);
  rc = rc ? rc : dalloc(ctx, &pl->d_out, (size_t)pl->nrec);
  rc = rc ? rc : dalloc(ctx, &pl->d_err, 4);
  if (pl->fst) rc = rc ? rc : dalloc(ctx, &pl->d_fst, (size_t)pl->nslots + 1);
  pl->d_fst_own = pl->d_fst;
  if ((pl->seg_search || pl->seg_index || slide) && !rc) {   // k_slots_search's / k_slots_index's / k_slots_slide's / k_slots_regions's slot bases per chromosome (u32: nslots < 2^31)
    std::vector<uint32_t> sb(pl->slot_base_h.begin(), pl->slot_base_h.end());
    rc = dalloc(ctx, &pl->d_slot_base, sb.size());
    if (!rc && hipMemcpy(pl->d_slot_base, sb.data(), sizeof(uint32_t) * sb.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = set_err(ctx, SFS2D_E_HIP, "slot bases upload");
  }
  if (rg && !rc) {   // k_slots_regions's (first, last) per slot: copied once, the caller's arrays are not kept
    std::vector<uint2> reg((size_t)rg->n);
    for (int64_t i = 0; i < rg->n; ++i) reg[(size_t)i] = make_uint2(rg->first[i], rg->last[i]);
    rc = dalloc(ctx, &pl->d_reg, reg.size());
    if (!rc && hipMemcpy(pl->d_reg, reg.data(), sizeof(uint2) * reg.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = set_err(ctx, SFS2D_E_HIP, "regions upload");
  }
  if (pl->fst) rc = rc ? rc : dalloc(ctx, &pl->d_fsum, 2 * ((size_t)pl->nslots + 1));
  if (rc) { plan_free(pl); delete pl; return rc; }
  hipError_t e = hipSuccess;
#define PCPY(dst, v) if (e == hipSuccess && !(v).empty()) e = hipMemcpyAsync(dst, (v).data(), sizeof((v)[0]) * (v).size(), hipMemcpyHostToDevice, st)
  PCPY(pl->d_tiles, pl->tiles);
  PCPY(pl->d_chunks, pl->chunks);
  PCPY(pl->d_leaves, pw.leaves);
  PCPY(pl->d_nodes, pw.nodes);
  PCPY(pl->d_slices, pl->slices);
#undef PCPY
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_slots, 0, sizeof(uint2) * ((size_t)pl->nslots + 1), st);
  if (e == hipSuccess && pl->do_bg) e = hipMemsetAsync(pl->d_repl, 0, sizeof(uint32_t) * nrepl, st);
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_bcount, 0, sizeof(uint32_t) * 2 * std::max(1, nc), st);
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_done, 0, sizeof(uint32_t) * pl->nbg, st);
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_ctr, 0, sizeof(uint32_t) * nctr, st);
  if (e == hipSuccess && pl->gw) e = hipMemsetAsync(pl->d_gscr, 0, sizeof(uint32_t) * ngscr, st);
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_err, 0, 4 * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_bins, 0, sizeof(uint32_t) * nbins, st);
  if (e == hipSuccess && pl->fst) e = hipMemsetAsync(pl->d_fsum, 0, sizeof(unsigned long long) * 2 * ((size_t)pl->nslots + 1), st);
  if (e == hipSuccess) e = hipMemsetAsync(pl->d_out, 0, sizeof(sfs2d_window) * (size_t)pl->nrec, st);
  for (auto& ev : pl->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    plan_free(pl); delete pl;
    return set_err(ctx, SFS2D_E_HIP, std::string("plan setup: ") + hipGetErrorString(e));
  }
  pl->bg_ready = false;
  *out = pl;
  return 0;
}

int64_t sfs2d_plan_num_records(const sfs2d_plan* pl) { return pl ? pl->nrec : -1; }

int sfs2d_plan_set_background(sfs2d_plan* pl, const double* bg2d, const double* bg1a, const double* bg1b) {
  if (!pl || !bg2d || !bg1a || !bg1b) return set_err(pl ? pl->ctx : nullptr, SFS2D_E_ARG, "null argument");
  sfs2d_ctx* ctx = pl->ctx;
  if (pl->prm.bg_mode != SFS2D_BG_SUPPLIED) return set_err(ctx, SFS2D_E_ARG, "plan does not take a supplied background");
  const KParams& K = pl->K;
  std::vector<double> v(K.nt);
  std::memcpy(v.data(), bg2d, sizeof(double) * K.nb2);
  std::memcpy(v.data() + K.t1a, bg1a, sizeof(double) * (K.n1p + 1));
  std::memcpy(v.data() + K.t1b, bg1b, sizeof(double) * (K.n2p + 1));
  bool integer_values = true;
  for (double x : v)
    if (!(x == std::floor(x)) || std::fabs(x) > 9.0e15) { integer_values = false; break; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(pl->d_bgval, v.data(), sizeof(double) * K.nt, hipMemcpyHostToDevice, CTX_STREAM(ctx)));
  HIPCHK(ctx, launch_finalize(pl, integer_values ? 1 : 0));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  pl->bg_ready = true;
  return 0;
}

int sfs2d_plan_run_phase(sfs2d_plan* pl, int phase, sfs2d_window* out_dev) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  if (pl->base) return set_err(ctx, SFS2D_E_ARG, "an attached plan runs with its base plan (sfs2d_plan_attach)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // a sampled run split into phases 1 and 2 (sfs2d_plan_run_streams' staggered first run) keeps
  // its events from phase 1 to phase 2 (tpend)
  hipEvent_t* te = nullptr;
  if (phase == 2) {
    te = pl->tpend;
    pl->tpend = nullptr;
  } else if (pl->timing && (pl->tseen++ % pl->tevery) == 0 && pl->tcount < pl->tmax) {
    te = &pl->tev[(size_t)pl->tcount * 6];
  }
  if (!pl->do_bg && !pl->bg_ready && phase != 1)
    return set_err(ctx, SFS2D_E_ARG, "supplied-background plan run before sfs2d_plan_set_background");
  // sampled runs: each kernel carries its start / end events in its own dispatch packet; a kernel
  // this run does not launch gets both events recorded in the stream instead (duration ~0)
  for (int k = 0; k < 6; ++k) pl->kev[k] = (te && ((pl->tmask >> (k / 2)) & 1)) ? te[k] : nullptr;
  auto mark = [&](int k) -> int {
    if (te && ((pl->tmask >> (k / 2)) & 1)) {
      HIPCHK(ctx, hipEventRecord(te[k], CTX_STREAM(ctx)));
      HIPCHK(ctx, hipEventRecord(te[k + 1], CTX_STREAM(ctx)));
    }
    return 0;
  };
  int rc = 0;
  if (phase == 0 || phase == 1) {
    if (slots_only(pl)) {
      HIPCHK(ctx, launch_slots_only(pl));
      if (pl->nslots == 0 && (rc = mark(0))) return rc;
    } else {
      if (pl->seg_index) HIPCHK(ctx, stage_slots(pl));
      if ((rc = launch_prep(pl, true))) return rc;
      const bool slots = free_slots(pl) && pl->nslots;   // a sliding / regions plan's table, after k_prep
      if (slots) HIPCHK(ctx, launch_slots_slide(pl, !prep_runs(pl)));
      if (!prep_runs(pl) && !slots && (rc = mark(0))) return rc;
    }
  }
  if (phase == 0 || phase == 2) {
    if (pl->do_bg && !pl->fused) HIPCHK(ctx, launch_bg_slices(pl));
    else if ((rc = mark(2))) return rc;
    if (free_slots(pl) && pl->fst_win) HIPCHK(ctx, launch_fst_win(pl));   // (the scan may clear the slots)
    for (sfs2d_plan* a : pl->attached)   // before the base clears its state
      if ((rc = launch_attached(a))) return rc;
    sfs2d_window* out = out_dev ? out_dev : pl->d_out;
    if (pl->chunks.empty() && (rc = mark(4))) return rc;
    if ((rc = launch_scan_any(pl, out))) return rc;
    pl->last_out = out;
    pl->runs++;
    if (!ctx->capturing) pl->done++;
  }
  for (auto& e : pl->kev) e = nullptr;
  if (te && phase == 1) pl->tpend = te;   // (counted when its phase 2 has run)
  else if (te) pl->tcount++;
  return 0;
}

int sfs2d_plan_grids(const sfs2d_plan* pl, int64_t* prep_threads, int64_t* scan_threads) {
  if (!pl) return SFS2D_E_ARG;
  if (prep_threads) *prep_threads = (int64_t)pl->tiles.size() * BLOCK1;
  if (scan_threads) *scan_threads = (int64_t)pl->chunks.size() * (pl->G == WAVE ? SBLOCK : pl->gw ? WAVE : BLOCK);
  return 0;
}

const char* sfs2d_plan_scan_kernel(const sfs2d_plan* pl) {
  if (!pl) return nullptr;
  if (pl->gw) return "k_scan_gw";
  return pl->G == WAVE ? "k_scan_w" : "k_scan_g";
}

const char* sfs2d_plan_seg_kind(const sfs2d_plan* pl) {
  if (!pl) return nullptr;
  if (pl->regions) return "regions";
  if (pl->base) return pl->step ? "slide" : pl->prm.window_mode == SFS2D_WINDOW_BP ? "bp" : "none";
  if (pl->step) return "slide";
  if (pl->seg_index) return "index";
  if (slots_only(pl)) return pl->seg_synth ? "synth" : "search";
  return pl->do_seg ? "prep" : "none";
}

int sfs2d_plan_slots_once(const sfs2d_plan* pl) { return !pl ? SFS2D_E_ARG : pl->slots_once ? 1 : 0; }

int sfs2d_plan_scan_variant(const sfs2d_plan* pl, int* p16, int* fused, int* fst, int* cnt, int* gate, int* tri) {
  if (!pl) return SFS2D_E_ARG;
  if (!pl->variant_set) return set_err(pl->ctx, SFS2D_E_ARG, "sfs2d_plan_scan_variant: the plan has launched no scan kernel yet");
  int* const o[6] = {p16, fused, fst, cnt, gate, tri};
  for (int i = 0; i < 6; ++i)
    if (o[i]) *o[i] = pl->variant[i];
  return 0;
}

int sfs2d_plan_scan_packing(const sfs2d_plan* pl, int* tri, int* sb, int* r1) {
  if (!pl) return SFS2D_E_ARG;
  const bool w = pl->G == WAVE && !pl->gw;
  if (tri) *tri = w ? (pl->tri ? 1 : 0) : -1;
  if (sb) *sb = w ? pl->sb : -1;
  if (r1) *r1 = w ? pl->r1 : -1;
  return 0;
}

int sfs2d_plan_set_timing(sfs2d_plan* pl, int max_runs) { return sfs2d_plan_set_timing_sampled(pl, max_runs, 1); }

int sfs2d_plan_set_timing_sampled(sfs2d_plan* pl, int max_runs, int every) {
  return sfs2d_plan_set_timing_kernels(pl, max_runs, every, 7);
}

int sfs2d_plan_set_timing_kernels(sfs2d_plan* pl, int max_runs, int every, int kernel_mask) {
  if (!pl || max_runs < 0 || every < 1 || (kernel_mask & ~7) || !kernel_mask) return SFS2D_E_ARG;
  pl->tevery = every;
  pl->tmask = kernel_mask;
  pl->tseen = 0;
  sfs2d_ctx* ctx = pl->ctx;
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  // the event ring only grows (turning timing off keeps it): re-arming a sampled loop then costs no
  // event creation -- hundreds of hipEventCreate calls right before a timed loop left the GPU idle for
  // milliseconds first
  if ((size_t)max_runs * 6 > pl->tev.size()) {
    for (auto& e : pl->tev) if (e) hipEventDestroy(e);
    pl->tev.assign((size_t)max_runs * 6, nullptr);
    for (auto& e : pl->tev) HIPCHK(ctx, hipEventCreate(&e));
  }
  pl->tmax = max_runs;
  pl->tcount = 0;
  pl->tpend = nullptr;
  pl->timing = max_runs > 0;
  return 0;
}

int sfs2d_plan_timing_read(sfs2d_plan* pl, int* nruns, double* ms_k1, double* ms_k2, double* ms_k3) {
  if (!pl || !nruns) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  double t[3] = {0, 0, 0};
  const int klast = (pl->tmask & 4) ? 2 : (pl->tmask & 2) ? 1 : 0;   // the run's last recorded event pair
  for (int r = 0; r < pl->tcount; ++r) {
    hipEvent_t* te = &pl->tev[(size_t)r * 6];
    HIPCHK(ctx, hipEventSynchronize(te[2 * klast + 1]));
    for (int k = 0; k < 3; ++k) {
      if (!((pl->tmask >> k) & 1)) continue;
      float ms = 0;
      HIPCHK(ctx, hipEventElapsedTime(&ms, te[2 * k], te[2 * k + 1]));
      t[k] += ms;
    }
  }
  *nruns = pl->tcount;
  const double d = pl->tcount ? pl->tcount : 1;
  if (ms_k1) *ms_k1 = t[0] / d;
  if (ms_k2) *ms_k2 = t[1] / d;
  if (ms_k3) *ms_k3 = t[2] / d;
  return 0;
}

int sfs2d_plan_run(sfs2d_plan* pl, sfs2d_window* out_dev) { return sfs2d_plan_run_phase(pl, 0, out_dev); }

int sfs2d_plan_run_many(sfs2d_plan* pl, int nruns, sfs2d_window* out_dev) {
  if (!pl || nruns < 0) return SFS2D_E_ARG;
  for (int i = 0; i < nruns; ++i) {
    const int rc = sfs2d_plan_run_phase(pl, 0, out_dev);
    if (rc) return rc;
  }
  return 0;
}

int sfs2d_plan_run_streams(sfs2d_plan* const* plans, void* const* streams, sfs2d_window* const* outs, int nplans,
                           int nruns) {
  if (!plans || !streams || nplans < 1 || nruns < 0) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = plans[0] ? plans[0]->ctx : nullptr;
  if (!ctx) return SFS2D_E_ARG;
  for (int k = 0; k < nplans; ++k) {
    if (!plans[k] || plans[k]->ctx != ctx) return set_err(ctx, SFS2D_E_ARG, "plans must share one ctx");
    for (int j = 0; j < k; ++j)
      if (plans[j] == plans[k]) return set_err(ctx, SFS2D_E_ARG, "a plan may appear once (its per-run state is not shareable)");
  }
  // run i: plan i % nplans on stream i % nplans.  The plans' per-run state (bins, replicas, slots,
  // counters) is their own, so consecutive runs on different streams overlap.  (One host thread
  // enqueues: config 2 with 3 streams is not host-bound -- 10.7 us of enqueue per pass vs 14.5 us on
  // the GPU; a thread per stream gained 1.5% at 400 passes and lost its thread starts in 20-pass runs,
  // profiles/r02i_enqueue_probe.txt)
  // The streams start staggered: the second stream's first run waits for the first run's k_prep, so
  // that from the start one stream's bandwidth-bound k_prep runs beside the other's latency-bound scan
  // (started together, the two k_preps competed and then the two scans, and the streams kept that
  // phase: config 3's 20-step bench loop 0.184 vs 0.190-0.198 ms per pass, without Fst 0.165 vs 0.181;
  // profiles/r05u_stream_stagger_ab.txt).  Not for plans with attached plans: their longer passes
  // settled into a worse phase staggered (20 kb + 500 kb: 0.328-0.331 vs 0.285-0.286 ms per step).
  // Chaining every run's k_prep after the previous run's k_prep (and its scan after the previous scan)
  // measured slower: 0.1852-0.1857 (0.238-0.248) vs 0.1821-0.1828 ms (profiles/r06l_stream_chain_ab.txt).
  // About one 20-run loop in eight settles into a slower phase (0.19-0.216 ms per run, the scans of both
  // streams overlapping more); the k_prep chain never did in 8 runs but costs ~2% in the typical one, a
  // chained start made the slow phase likelier (5 of 8), the scan chain is far slower
  // (profiles/r06v_*, r06w_*, r06x_*)
  bool stagger = nplans >= 2 && nruns >= 2;
  for (int k = 0; k < nplans; ++k) stagger = stagger && plans[k]->attached.empty();
  if (stagger && !ctx->stagger) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->stagger, hipEventDisableTiming));
  hipStream_t saved = CTX_STREAM(ctx);
  int rc = 0;
  for (int i = 0; i < nruns && !rc; ++i) {
    const int k = i % nplans;
    ctx->stream = (hipStream_t)streams[k];   // (NULL: the null stream, as sfs2d_ctx_set_stream)
    if (stagger && i == 0) {
      rc = sfs2d_plan_run_phase(plans[k], 1, outs ? outs[k] : nullptr);
      if (!rc && hipEventRecord(ctx->stagger, ctx->stream) != hipSuccess) rc = set_err(ctx, SFS2D_E_HIP, "stagger event");
      if (!rc) rc = sfs2d_plan_run_phase(plans[k], 2, outs ? outs[k] : nullptr);
      continue;
    }
    if (stagger && i == 1 && hipStreamWaitEvent(ctx->stream, ctx->stagger, 0) != hipSuccess)
      rc = set_err(ctx, SFS2D_E_HIP, "stagger wait");
    if (!rc) rc = sfs2d_plan_run_phase(plans[k], 0, outs ? outs[k] : nullptr);
  }
  ctx->stream = saved;
  return rc;
}

// A run_streams sequence captured into HIP graphs, one per stream (each a chain of its plans' runs), and
// replayed with one hipGraphLaunch per stream: short passes (config 2's 1e6-SNP chromosome, ~12 us of
// GPU time per pass) are host-bound when each of their three launches is enqueued on its own.  One graph
// holding all the streams' chains as parallel branches (forked and joined through events) measured 6-9x
// slower than run_streams (0.066-0.107 vs 0.0117 ms per pass, profiles/r06ad_*): the replay does not
// overlap the branches the way independent streams do.  The runs' kernel arguments (parity-selected
// buffers, output pointers) are fixed at capture: every plan runs an even number of times per replay, so
// its buffer parity is the same before and after each replay, and a replay refuses to start when a plan
// ran an odd number of times since the capture.
struct sfs2d_graph {
  sfs2d_ctx* ctx = nullptr;
  std::vector<hipStream_t> streams;
  std::vector<hipGraph_t> graphs;
  std::vector<hipGraphExec_t> execs;
  std::vector<sfs2d_plan*> plans;
  std::vector<int64_t> par;
  std::vector<sfs2d_window*> outs;   // where a replay leaves each plan's records (the plan's last_out after a launch)
  uint64_t per_plan = 0;             // runs of every plan in one replay
};

static void graph_free(sfs2d_graph* g) {
  for (auto& x : g->execs) if (x) hipGraphExecDestroy(x);
  for (auto& x : g->graphs) if (x) hipGraphDestroy(x);
  delete g;
}

int sfs2d_graph_create(sfs2d_plan* const* plans, void* const* streams, sfs2d_window* const* outs, int nplans,
                       int nruns, sfs2d_graph** out) {
  if (!plans || !streams || !out || nplans < 1 || nruns < 1) return SFS2D_E_ARG;
  *out = nullptr;
  sfs2d_ctx* ctx = plans[0] ? plans[0]->ctx : nullptr;
  if (!ctx) return SFS2D_E_ARG;
  if (nruns % (2 * nplans))
    return set_err(ctx, SFS2D_E_ARG, "a graph holds an even number of runs of every plan (nruns % (2 * nplans) == 0)");
  for (int k = 0; k < nplans; ++k) {
    if (!plans[k] || plans[k]->ctx != ctx) return set_err(ctx, SFS2D_E_ARG, "plans must share one ctx");
    for (int j = 0; j < k; ++j)
      if (plans[j] == plans[k]) return set_err(ctx, SFS2D_E_ARG, "a plan may appear once (its per-run state is not shareable)");
    if (plans[k]->timing) return set_err(ctx, SFS2D_E_ARG, "a plan with timing on cannot be captured");
    if (plans[k]->base) return set_err(ctx, SFS2D_E_ARG, "an attached plan runs with its base plan (sfs2d_plan_attach)");
    if (!streams[k]) return set_err(ctx, SFS2D_E_ARG, "graph capture needs non-null streams");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  sfs2d_graph* g = new sfs2d_graph;
  g->ctx = ctx;
  for (int k = 0; k < nplans; ++k) {
    hipStream_t s = (hipStream_t)streams[k];
    if (std::find(g->streams.begin(), g->streams.end(), s) == g->streams.end()) g->streams.push_back(s);
  }
  hipStream_t saved = CTX_STREAM(ctx);
  int rc = 0;
  hipError_t e = hipSuccess;
  // the capture enqueues nothing for execution: the plans' last runs, and where their records are, stay what they were
  std::vector<sfs2d_window*> last((size_t)nplans);
  for (int k = 0; k < nplans; ++k) last[(size_t)k] = plans[k]->last_out;
  // a slots_once plan that has not run yet writes its slot table now, on its stream and ahead of the capture
  // (synchronised below): the graphs then hold no slot kernel
  for (int k = 0; k < nplans && k < nruns && e == hipSuccess; ++k)
    if (plans[k]->seg_index && plans[k]->slots_once && !plans[k]->slots_written) {
      ctx->stream = (hipStream_t)streams[k];
      e = stage_slots(plans[k]);
    }
  for (hipStream_t s : g->streams) {
    if (e != hipSuccess) break;
    // run i of the sequence is plan i % nplans on its stream: this stream's chain, in sequence order
    e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) break;
    ctx->stream = s;
    ctx->capturing = true;
    for (int i = 0; i < nruns && !rc; ++i) {
      const int k = i % nplans;
      if ((hipStream_t)streams[k] == s) rc = sfs2d_plan_run_phase(plans[k], 0, outs ? outs[k] : nullptr);
    }
    ctx->capturing = false;
    hipGraph_t gr = nullptr;
    e = hipStreamEndCapture(s, &gr);
    g->graphs.push_back(gr);
    hipGraphExec_t x = nullptr;
    if (!rc && e == hipSuccess) e = hipGraphInstantiate(&x, gr, nullptr, nullptr, 0);
    g->execs.push_back(x);
    if (rc || e != hipSuccess) break;
  }
  ctx->stream = saved;
  for (int k = 0; k < nplans; ++k) {
    g->outs.push_back(outs && outs[k] ? outs[k] : plans[k]->d_out);
    plans[k]->last_out = last[(size_t)k];
  }
  if (rc || e != hipSuccess) {
    graph_free(g);
    return rc ? rc : set_err(ctx, SFS2D_E_HIP, std::string("graph capture: ") + hipGetErrorString(e));
  }
  g->per_plan = (uint64_t)(nruns / nplans);
  for (int k = 0; k < nplans; ++k) {
    g->plans.push_back(plans[k]);
    g->par.push_back(plans[k]->runs & 1);
  }
  *out = g;
  return 0;
}

int sfs2d_graph_launch(sfs2d_graph* g, int nlaunch) {
  if (!g || nlaunch < 0) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = g->ctx;
  for (size_t k = 0; k < g->plans.size(); ++k)
    if ((g->plans[k]->runs & 1) != g->par[k])
      return set_err(ctx, SFS2D_E_ARG, "a captured plan ran an odd number of times since the capture");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < nlaunch; ++i) {
    for (size_t j = 0; j < g->execs.size(); ++j) HIPCHK(ctx, hipGraphLaunch(g->execs[j], g->streams[j]));
    // the replay's runs are every captured plan's last runs now (host bookkeeping alone: nothing is synchronised)
    for (size_t k = 0; k < g->plans.size(); ++k) {
      sfs2d_plan* pl = g->plans[k];
      pl->done += g->per_plan;
      pl->last_out = g->outs[k];
      for (sfs2d_plan* a : pl->attached) a->done += g->per_plan;
    }
  }
  return 0;
}

int sfs2d_graph_destroy(sfs2d_graph* g) {
  if (!g) return SFS2D_E_ARG;
  hipSetDevice(g->ctx->device);
  for (hipStream_t s : g->streams) hipStreamSynchronize(s);   // (no replay in flight)
  graph_free(g);
  return 0;
}

int sfs2d_plan_bg_buffer(sfs2d_plan* pl, void** dev_ptr, int64_t* nbytes) {
  if (!pl || !dev_ptr || !nbytes) return SFS2D_E_ARG;
  // the replica buffer the next run's k_prep accumulates into (fused plans alternate two)
  *dev_ptr = pl->d_repl + (size_t)repl_par(pl) * REPL * pl->data->nchrom * pl->K.nh;
  *nbytes = pl->do_bg ? (int64_t)REPL * pl->data->nchrom * pl->K.nh * 4 : 0;
  return 0;
}

int sfs2d_plan_bg_words(const sfs2d_plan* pl, int64_t* replicas, int64_t* nchrom, int64_t* bins) {
  if (!pl || !replicas || !nchrom || !bins) return SFS2D_E_ARG;
  *replicas = pl->do_bg ? REPL : 0;
  *nchrom = pl->do_bg ? pl->data->nchrom : 0;
  *bins = pl->do_bg ? pl->K.nh : 0;
  return 0;
}

int sfs2d_plan_bg_exchange(sfs2d_plan* pl, uint32_t* host_repl, uint32_t* host_sums, int to_device) {
  if (!pl || !host_repl || !host_sums) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  if (!pl->do_bg) return set_err(ctx, SFS2D_E_ARG, "plan has no per-chromosome backgrounds");
  if (pl->base) return set_err(ctx, SFS2D_E_ARG, "exchange the base plan's backgrounds");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // this run's buffers: the replicas k_prep accumulated into and the per-chromosome inner 2D sums
  // (the parities of sfs2d_plan_run_phase(plan, 1) of the run in progress)
  uint32_t* r = pl->d_repl + (size_t)repl_par(pl) * REPL * pl->data->nchrom * pl->K.nh;
  uint32_t* b = pl->d_bcount + (size_t)plan_par(pl) * pl->K.nchrom;
  const size_t nr = (size_t)REPL * pl->data->nchrom * pl->K.nh * 4, nb = (size_t)pl->K.nchrom * 4;
  hipStream_t st = CTX_STREAM(ctx);
  if (to_device) {
    HIPCHK(ctx, hipMemcpyAsync(r, host_repl, nr, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(b, host_sums, nb, hipMemcpyHostToDevice, st));
  } else {
    HIPCHK(ctx, hipMemcpyAsync(host_repl, r, nr, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(host_sums, b, nb, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

int sfs2d_plan_bg_rows_dev(sfs2d_plan* pl, int64_t* d_rows, int64_t row_stride) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  if (!pl->do_bg) return set_err(ctx, SFS2D_E_ARG, "plan has no per-chromosome backgrounds");
  if (pl->base) return set_err(ctx, SFS2D_E_ARG, "exchange the base plan's backgrounds");
  const int W = pl->K.h1b + pl->K.n2 + 2;
  if (!d_rows || row_stride < W) return set_err(ctx, SFS2D_E_ARG, "rows: null or stride < SFS2D_BG_ROW_WORDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int nc = pl->data->nchrom;
  if (nc == 0) return 0;
  const size_t rs = (size_t)nc * pl->K.nh;
  hipLaunchKernelGGL(k_bg_rows_get, dim3((unsigned)((W + 255) / 256), (unsigned)nc), dim3(256), 0, CTX_STREAM(ctx), pl->K,
                     pl->d_repl + (size_t)repl_par(pl) * REPL * rs, (unsigned long long)rs,
                     pl->d_bcount + (size_t)plan_par(pl) * pl->K.nchrom, (long long*)d_rows, (long long)row_stride);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int sfs2d_plan_bg_rows_set_dev(sfs2d_plan* pl, const int64_t* d_rows, int64_t row_stride) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  if (!pl->do_bg) return set_err(ctx, SFS2D_E_ARG, "plan has no per-chromosome backgrounds");
  if (pl->base) return set_err(ctx, SFS2D_E_ARG, "exchange the base plan's backgrounds");
  const int W = pl->K.h1b + pl->K.n2 + 2;
  if (!d_rows || row_stride < W) return set_err(ctx, SFS2D_E_ARG, "rows: null or stride < SFS2D_BG_ROW_WORDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int nc = pl->data->nchrom;
  if (nc == 0) return 0;
  const size_t rs = (size_t)nc * pl->K.nh;
  const int nk = std::max(W, pl->K.nh);
  hipLaunchKernelGGL(k_bg_rows_set, dim3((unsigned)((nk + 255) / 256), (unsigned)nc), dim3(256), 0, CTX_STREAM(ctx), pl->K,
                     pl->d_repl + (size_t)repl_par(pl) * REPL * rs, (unsigned long long)rs,
                     pl->d_bcount + (size_t)plan_par(pl) * pl->K.nchrom, (const long long*)d_rows, (long long)row_stride,
                     pl->d_err);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int sfs2d_plan_fst_buffer(sfs2d_plan* pl, void** dev_ptr, int64_t* nslots) {
  if (!pl || !dev_ptr || !nslots) return SFS2D_E_ARG;
  if (!pl->fst) return set_err(pl->ctx, SFS2D_E_ARG, "plan was created without SFS2D_F_FST");
  *dev_ptr = pl->d_fst;
  *nslots = pl->nslots;
  return 0;
}

int sfs2d_plan_set_fst_out(sfs2d_plan* pl, double* d_fst) {
  if (!pl) return SFS2D_E_ARG;
  if (!pl->fst) return set_err(pl->ctx, SFS2D_E_ARG, "plan was created without SFS2D_F_FST");
  if (pl->base) return set_err(pl->ctx, SFS2D_E_ARG, "an attached plan's Fst buffer is its own");
  pl->d_fst = d_fst ? d_fst : pl->d_fst_own;
  return 0;
}

int sfs2d_plan_fst_read(sfs2d_plan* pl, double* out_host, int64_t cap) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  if (!pl->fst) return set_err(ctx, SFS2D_E_ARG, "plan was created without SFS2D_F_FST");
  if (pl->done == 0)
    return set_err(ctx, SFS2D_E_ARG, "Fst read before the plan's first run (a captured run counts once its graph is launched)");
  if (cap < pl->nslots) return set_err(ctx, SFS2D_E_CAP, "output capacity too small");
  if (pl->nslots && !out_host) return SFS2D_E_ARG;
  if (pl->nslots)
    HIPCHK(ctx, hipMemcpyAsync(out_host, pl->d_fst, sizeof(double) * pl->nslots, hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  return 0;
}

int sfs2d_plan_check(sfs2d_plan* pl) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  uint32_t e = 0;
  HIPCHK(ctx, hipMemcpyAsync(&e, pl->d_err, 4, hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  if (e) {
    HIPCHK(ctx, hipMemsetAsync(pl->d_err, 0, 4, CTX_STREAM(ctx)));
    HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
    if (e & ERR_OVF) return set_err(ctx, SFS2D_E_ARG, "summed background histograms overflow uint32");
    if (e & ERR_KEY) return set_err(ctx, SFS2D_E_KEY, "allele count above 2*pop_size (reference: KeyError in calculate_1d_sfs)");
    return set_err(ctx, SFS2D_E_GRID, "folded 2D bin outside the (2n1+1)x(2n2+1) grid");
  }
  return 0;
}

// diagnostic: stamps of a -DSFS2D_STAMPS build (returns SFS2D_E_ARG in the shipped build)
int sfs2d__debug_stamps(unsigned long long* out64) {
#ifdef SFS2D_STAMPS
  // 64 phase stamps, then per-block (start, end) of k_prep and k_scan_w (2 x 4096 x 2), then per wave,
  // then k_bg_slice per block
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 64) != hipSuccess) return SFS2D_E_HIP;
  if (hipMemcpyFromSymbol(out64 + 64, HIP_SYMBOL(g_blk), sizeof(unsigned long long) * 2 * 4096 * 2) != hipSuccess)
    return SFS2D_E_HIP;
  // then k_scan_w per wavefront (end, windows): 4096 x 8 x 2
  if (hipMemcpyFromSymbol(out64 + 64 + 2 * 4096 * 2, HIP_SYMBOL(g_wv), sizeof(unsigned long long) * 4096 * 8 * 2) != hipSuccess)
    return SFS2D_E_HIP;
  // then k_bg_slice per block (start, work done): 1024 x 2
  if (hipMemcpyFromSymbol(out64 + 64 + 2 * 4096 * 2 + 4096 * 8 * 2, HIP_SYMBOL(g_bgs), sizeof(unsigned long long) * 1024 * 2) != hipSuccess)
    return SFS2D_E_HIP;
  return 0;
#else
  (void)out64;
  return SFS2D_E_ARG;
#endif
}

int sfs2d_plan_stats(sfs2d_plan* pl, uint32_t* exact_windows) {
  if (!pl || !exact_windows) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  HIPCHK(ctx, hipMemcpyAsync(exact_windows, pl->d_err + 1, 4, hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  return 0;
}

int sfs2d_plan_read(sfs2d_plan* pl, sfs2d_window* out_host, int64_t cap, int64_t* nrec_out) {
  if (!pl || !nrec_out) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  *nrec_out = pl->nrec;
  if (pl->done == 0)
    return set_err(ctx, SFS2D_E_ARG, "read before the plan's first run (no records yet; a captured run counts once its graph "
                                     "is launched)");
  if (cap < pl->nrec) return set_err(ctx, SFS2D_E_CAP, "output capacity too small");
  if (pl->nrec && !out_host) return SFS2D_E_ARG;
  if (pl->nrec)
    HIPCHK(ctx, hipMemcpyAsync(out_host, last_records(pl), sizeof(sfs2d_window) * pl->nrec, hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  return 0;
}

// ------------------------------------------------------------------------------------------ post-scan calls
// The calls below work on the records of a plan's last executed run and share one skeleton ("post-scan
// calls: the common skeleton"): post_ready -- the plan has run, 32-bit SNP indices, the device, the last run's
// records; the selection (sel_shape, sel_rows_fit, sel_walk); device arrays that grow on demand (reserve) and the
// call's result in the caller's buffer or the plan's own (call_out); the LDS grant (grant_lds); the launch; and
// the read of what the last call wrote (read_ready, read_last).

extern "C++" {
namespace {

// What a post-scan call needs before it looks at its own arguments: the plan has run (a run that was only captured
// has not executed: sfs2d_graph_launch counts it), SNP indices fit 32 bits and the device is current.  *recs: the
// last run's records.  unrun: the call's own words for a plan that has not run (the null's).
int post_ready(sfs2d_plan* pl, const char* name, const sfs2d_window** recs, const char* unrun = nullptr) {
  sfs2d_ctx* ctx = pl->ctx;
  if (pl->done == 0)
    return set_err(ctx, SFS2D_E_ARG,
                   unrun ? std::string(unrun)
                         : std::string(name) + (pl->base ? " before the base plan's first run (an attached plan has no records yet)"
                                                         : " before the plan's first run (no records yet)"));
  if (pl->data->n > 0xffffffffll)
    return set_err(ctx, SFS2D_E_ARG, std::string(name) + ": data set too large for 32-bit SNP indices");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  *recs = last_records(pl);
  return 0;
}

// The shape of a selection (rec, grp, nsel, ngroups) of sfs2d_plan_spectra and sfs2d_plan_project ...
int sel_shape(sfs2d_plan* pl, const std::string& name, const int64_t* rec, const int32_t* grp, int64_t nsel,
              int64_t ngroups) {
  sfs2d_ctx* ctx = pl->ctx;
  if (nsel < 0) return set_err(ctx, SFS2D_E_ARG, name + ": nsel must be >= 0");
  if (ngroups < 1) return set_err(ctx, SFS2D_E_ARG, name + ": ngroups must be >= 1");
  if (!rec && nsel != pl->nrec)
    return set_err(ctx, SFS2D_E_ARG, name + ": rec == NULL selects every record in order: nsel must be the plan's record count");
  if (rec && !grp) return set_err(ctx, SFS2D_E_ARG, name + ": grp == NULL needs rec == NULL (group i = record i)");
  if (nsel > 0xffffffffll) return set_err(ctx, SFS2D_E_ARG, name + ": more than 2^32 - 1 selection entries");
  if (!grp && nsel > ngroups)
    return set_err(ctx, SFS2D_E_ARG, name + ": group i = record i needs ngroups >= the plan's record count");
  return 0;
}
// ... its rows, ngroups x roww int64 words, in 64 bits (the two calls ask at different points: spectra after the
// entries, project before them, so an argument set with two faults is refused for the same one as ever) ...
int sel_rows_fit(sfs2d_plan* pl, const std::string& name, int64_t ngroups, int64_t roww) {
  if (ngroups > 0xffffffffll || ngroups > (INT64_MAX / 8) / roww)
    return set_err(pl->ctx, SFS2D_E_NOMEM, name + ": " + std::to_string(ngroups) + " rows of " + std::to_string(roww) +
                                               " int64 words do not fit");
  return 0;
}
// ... and its entries: entry(i, r, g) for entry i of record r in [0, nrec) and group g in [0, ngroups), its return
// value other than 0 ending the walk.  neg: a negative r is the callback's to judge (project's chromosome
// entries); such a call names a bad group before a bad record, the other a bad record first.
template <class Entry>
int sel_walk(sfs2d_plan* pl, const std::string& name, const int64_t* rec, const int32_t* grp, int64_t nsel,
             int64_t ngroups, bool neg, Entry entry) {
  sfs2d_ctx* ctx = pl->ctx;
  for (int64_t i = 0; i < nsel; ++i) {
    const int64_t r = rec ? rec[i] : i, g = grp ? (int64_t)grp[i] : i;
    const bool bad_r = r >= pl->nrec || (r < 0 && !neg), bad_g = g < 0 || g >= ngroups;
    if (bad_g && (neg || !bad_r))
      return set_err(ctx, SFS2D_E_ARG, name + ": entry " + std::to_string(i) + ": group " + std::to_string(g) +
                                           " outside [0, " + std::to_string(ngroups) + ")");
    if (bad_r)
      return set_err(ctx, SFS2D_E_ARG, name + ": entry " + std::to_string(i) + ": record " + std::to_string(r) +
                                           " outside [0, " + std::to_string(pl->nrec) + ")");
    const int rc = entry(i, r, g);
    if (rc) return rc;
  }
  return 0;
}

// b holds `want` elements: what it held is replaced when it is too small -- after the stream has been synchronised,
// once per call (*synced), since an earlier call may still read what is replaced.  A failed allocation leaves b
// empty and the HIP error cleared.
template <typename T>
int reserve(sfs2d_ctx* ctx, hipStream_t st, DevBuf<T>& b, size_t want, bool* synced) {
  if (want <= b.cap) return 0;
  if (b.p && !*synced) {
    HIPCHK(ctx, hipStreamSynchronize(st));
    *synced = true;
  }
  hipFree(b.p);
  b.cap = 0;
  const int rc = dalloc(ctx, &b.p, want);
  if (rc) (void)hipGetLastError();
  else b.cap = want;
  return rc;
}
// *out: where a call writes its n elements -- the caller's buffer, or the plan's own, which grows to hold them (the
// earlier result is then gone: no call yet)
template <typename T, int64_t NONE>
int call_out(sfs2d_ctx* ctx, hipStream_t st, CallOut<T, NONE>& o, T* out_dev, size_t n, bool* synced, T** out) {
  if (!out_dev && n > o.own.cap) {
    o.last = nullptr;
    o.n = NONE;
    const int rc = reserve(ctx, st, o.own, n, synced);
    if (rc) return rc;
  }
  *out = out_dev ? out_dev : o.own.p;
  return 0;
}

// the refusals of a read call -- no call yet, a capacity below the count, which *n_out reports either way -- ...
template <typename T, int64_t NONE>
int read_ready(sfs2d_plan* pl, const CallOut<T, NONE>& o, int64_t cap, int64_t* n_out, const char* name) {
  if (o.n < 0) return set_err(pl->ctx, SFS2D_E_ARG, std::string(name) + "_read before " + name);
  *n_out = o.n;
  if (cap < o.n) return set_err(pl->ctx, SFS2D_E_CAP, "output capacity too small");
  return 0;
}
// ... and the read itself: the elements the last call wrote, from where it wrote them (synchronises)
template <typename T, int64_t NONE>
int read_last(sfs2d_plan* pl, const CallOut<T, NONE>& o, T* host, int64_t cap, int64_t* n_out, const char* name) {
  sfs2d_ctx* ctx = pl->ctx;
  const int rc = read_ready(pl, o, cap, n_out, name);
  if (rc) return rc;
  if (o.n && !host) return SFS2D_E_ARG;
  if (o.n) HIPCHK(ctx, hipMemcpyAsync(host, o.last, sizeof(T) * (size_t)o.n, hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  return 0;
}

}  // namespace
}  // extern "C++"

// ------------------------------------------------------------------------------------------ bootstrap null

extern "C++" {
namespace {

// The tables k_null reads, complete for every chromosome.  Large-grid plans (k_bg_slice with its tail)
// and supplied backgrounds (k_bg_finalize) leave them after every run.  The small-grid scans keep their
// chromosome's finished table in LDS and store only the Q9 chromosome's, so:
//   sliced: k_bg_slice left the table, the leaf sums, the 1D results and the run's inner sums -- its
//           tail alone is missing (k_null_tail);
//   fused:  the last run's replicas and inner sums are still in their parity buffer (the next scan
//           clears them): k_bg_slice with its tail builds the tables from them.  It zeroes what it reads,
//           which the next scan would do anyway, so it runs once per plan run (null_tab_runs).
int null_tables(sfs2d_plan* pl) {
  sfs2d_ctx* ctx = pl->ctx;
  if (!pl->do_bg || !(pl->fused || pl->sliced) || pl->null_tab_runs == pl->done) return 0;
  const size_t lp = (size_t)((pl->runs - 1) & 1);   // parity of the last run
  if (pl->fused) {
    hipLaunchKernelGGL(k_bg_slice, dim3((unsigned)pl->slices.size() + 1, (unsigned)pl->nbg), dim3(KBLOCK), 0, CTX_STREAM(ctx),
                       pl->K, pl->d_repl + lp * REPL * pl->K.nchrom * pl->K.nh, pl->d_bcount + lp * pl->K.nchrom, pl->d_tab,
                       pl->d_lp, pl->d_head, pl->d_leafsum, pl->d_bg1d, pl->d_done, pl->d_slices, (int)pl->slices.size(),
                       pl->d_leaves, pl->nleaves, pl->d_nodes, pl->nnodes, pl->nlevels, 1, 0, pl->data->counts, scan_src(pl),
                       pl->d_slots, reinterpret_cast<const double2*>(ctx->d_df + 2 * LNT), pl->d_fst, (uint32_t)pl->nslots);
  } else {
    hipLaunchKernelGGL(k_null_tail, dim3((unsigned)pl->nbg), dim3(KBLOCK), 0, CTX_STREAM(ctx), pl->K,
                       pl->d_bcount + lp * pl->K.nchrom, pl->d_tab, pl->d_lp, pl->d_head, pl->d_leafsum, pl->d_bg1d,
                       pl->nleaves, pl->d_nodes, pl->nnodes, pl->nlevels);
  }
  HIPCHK(ctx, hipGetLastError());
  pl->null_tab_runs = pl->done;
  return 0;
}

// block == 1: k_null; a longer block: k_null_blk (the same LDS layout, workgroup and grid)
template <bool P16, bool CNT>
int launch_null(sfs2d_plan* pl, uint32_t R, unsigned long long nrec, uint2 key, uint32_t block, sfs2d_window* out) {
  sfs2d_ctx* ctx = pl->ctx;
  const KParams& K = pl->K;
  // wavefronts per workgroup from the LDS a wave's histograms need: as many as fit 64 KB, at most 8
  const size_t per = (size_t)null_wave_words(K.nb2, K.n1p, K.n2p, P16) * 4;
  const int wpb = (int)std::max<size_t>(1, std::min<size_t>(NULL_MAX_WAVES, (64 * 1024) / per));
  const size_t lds = per * wpb;
  if (lds > 160 * 1024) return set_err(ctx, SFS2D_E_ARG, "2D grid too large for k_null's LDS histogram");
  const void* f = block == 1u ? (const void*)k_null<P16, CNT> : (const void*)k_null_blk<P16, CNT>;
  if (lds > 64 * 1024) HIPCHK(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int occ = 0;
  const hipError_t oe = block == 1u ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_null<P16, CNT>, wpb * WAVE, lds)
                                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_null_blk<P16, CNT>, wpb * WAVE, lds);
  if (oe != hipSuccess || occ < 1) {
    (void)hipGetLastError();
    occ = 1;
  }
  // one resident set of workgroups striding over the records (a wave zeroes its histograms once)
  const unsigned long long want = (nrec + wpb - 1) / wpb;
  const unsigned grid = (unsigned)std::min<unsigned long long>(want, (unsigned long long)occ * ctx->ncu);
  if (block == 1u)
    hipLaunchKernelGGL((k_null<P16, CNT>), dim3(grid), dim3(wpb * WAVE), lds, CTX_STREAM(ctx), K, scan_src(pl), pl->ntask.p, R,
                       nrec, key, pl->d_tab, pl->d_head, pl->do_bg ? 1 : 0, ctx->d_lnx, out);
  else
    hipLaunchKernelGGL((k_null_blk<P16, CNT>), dim3(grid), dim3(wpb * WAVE), lds, CTX_STREAM(ctx), K, scan_src(pl),
                       pl->ntask.p, R, nrec, key, block, pl->d_tab, pl->d_head, pl->do_bg ? 1 : 0, ctx->d_lnx, out);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // namespace
}  // extern "C++"

int sfs2d_plan_null_run(sfs2d_plan* pl, const sfs2d_null_params* np, const int64_t* tasks, int64_t ntasks,
                        sfs2d_window* out_dev) {
  return sfs2d_plan_null_run_blocks(pl, np, 1, tasks, ntasks, out_dev);
}

int sfs2d_plan_null_run_blocks(sfs2d_plan* pl, const sfs2d_null_params* np, int64_t block, const int64_t* tasks,
                               int64_t ntasks, sfs2d_window* out_dev) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  if (!np || ntasks < 0 || (ntasks > 0 && !tasks)) return set_err(ctx, SFS2D_E_ARG, "null argument");
  if (block < 1 || block > 0xffffffffll)
    return set_err(ctx, SFS2D_E_ARG, "null run: block length " + std::to_string(block) + " must be in [1, 2^32)");
  if (pl->base) return set_err(ctx, SFS2D_E_ARG, "null run on an attached plan: use its base plan (same data, same tables)");
  const sfs2d_window* recs = nullptr;   // (not read: the null draws from the pools and the run's tables)
  int rc = post_ready(pl, "null run", &recs, "null run before the plan's first run (no background tables yet; a captured run "
                                             "counts once its graph is launched)");
  if (rc) return rc;
  if (np->replicates < 1) return set_err(ctx, SFS2D_E_ARG, "null run: replicates must be >= 1");
  pl->ntask_h.resize((size_t)ntasks);
  uint32_t maxm = 0;
  for (int64_t t = 0; t < ntasks; ++t) {
    const int64_t pool = tasks[2 * t], m = tasks[2 * t + 1];
    if (pool < -1 || pool >= d->nchrom) return set_err(ctx, SFS2D_E_ARG, "null run: pool " + std::to_string(pool) + " out of range");
    if (pool == -1 && pl->do_bg)
      return set_err(ctx, SFS2D_E_ARG, "null run: pool -1 (all SNPs) has no background on a per-chromosome plan");
    const int64_t lo = pool < 0 ? 0 : d->chrom_off[pool], hi = pool < 0 ? d->n : d->chrom_off[pool + 1];
    if (hi <= lo) return set_err(ctx, SFS2D_E_ARG, "null run: pool " + std::to_string(pool) + " is empty");
    if (m < 1 || m > 0xffffffffll) return set_err(ctx, SFS2D_E_ARG, "null run: m must be in [1, 2^32)");
    NullTask k;
    k.lo = (uint32_t)lo; k.n = (uint32_t)(hi - lo); k.m = (uint32_t)m; k.pool = (int32_t)pool;
    pl->ntask_h[(size_t)t] = k;
    maxm = std::max(maxm, k.m);
  }
  const unsigned long long nrec = (unsigned long long)ntasks * np->replicates;
  if (nrec > (1ull << 26)) return set_err(ctx, SFS2D_E_CAP, "null run: more than 2^26 records in one call (split the tasks)");
  hipStream_t st = CTX_STREAM(ctx);
  bool synced = false;
  sfs2d_window* out = nullptr;
  if ((rc = reserve(ctx, st, pl->ntask, (size_t)ntasks, &synced))) return rc;
  if ((rc = call_out(ctx, st, pl->null_out, out_dev, (size_t)nrec, &synced, &out))) return rc;
  pl->null_out.last = out;
  pl->null_out.n = (int64_t)nrec;
  if (nrec == 0) return 0;
  if ((rc = null_tables(pl))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(pl->ntask.p, pl->ntask_h.data(), sizeof(NullTask) * (size_t)ntasks, hipMemcpyHostToDevice, st));
  const uint2 key = make_uint2((uint32_t)np->seed, (uint32_t)(np->seed >> 32));
  // u16-packed 2D bins while no bin can hold 65536 draws
  const uint32_t blk = (uint32_t)block;
  if (maxm <= 65535u)
    return pl->cnt ? launch_null<true, true>(pl, np->replicates, nrec, key, blk, out)
                   : launch_null<true, false>(pl, np->replicates, nrec, key, blk, out);
  return pl->cnt ? launch_null<false, true>(pl, np->replicates, nrec, key, blk, out)
                 : launch_null<false, false>(pl, np->replicates, nrec, key, blk, out);
}

int sfs2d_plan_null_read(sfs2d_plan* pl, sfs2d_window* out_host, int64_t cap, int64_t* nrec_out) {
  if (!pl || !nrec_out) return SFS2D_E_ARG;
  return read_last(pl, pl->null_out, out_host, cap, nrec_out, "sfs2d_plan_null");
}

// ------------------------------------------------------------------------------------------ diversity

int sfs2d_plan_diversity(sfs2d_plan* pl, sfs2d_diversity* out_dev) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  const sfs2d_window* recs = nullptr;
  int rc = post_ready(pl, "diversity", &recs);
  if (rc) return rc;
  bool synced = false;
  sfs2d_diversity* out = nullptr;
  if ((rc = call_out(ctx, CTX_STREAM(ctx), pl->div_out, out_dev, (size_t)pl->nrec, &synced, &out))) return rc;
  pl->div_out.last = out;
  pl->div_out.n = pl->nrec;
  if (pl->nrec == 0) return 0;
  // one wavefront per record, four per workgroup, the records strided over at most 2048 workgroups (as k_fst_win)
  const uint32_t nrec = (uint32_t)pl->nrec;
  const dim3 g((unsigned)std::min<uint32_t>(2048u, (nrec + 3u) / 4u));
  const double2* rt = reinterpret_cast<const double2*>(ctx->d_df + 2 * LNT);
  if (pl->cnt)
    hipLaunchKernelGGL(k_div_win<true>, g, dim3(DIV_BLOCK), 0, CTX_STREAM(ctx), pl->K, d->counts, scan_src(pl), recs, rt,
                       ctx->d_hw, out, nrec, (uint32_t)d->n);
  else
    hipLaunchKernelGGL(k_div_win<false>, g, dim3(DIV_BLOCK), 0, CTX_STREAM(ctx), pl->K, d->counts, scan_src(pl), recs, rt,
                       ctx->d_hw, out, nrec, (uint32_t)d->n);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int sfs2d_plan_diversity_read(sfs2d_plan* pl, sfs2d_diversity* out_host, int64_t cap, int64_t* nrec_out) {
  if (!pl || !nrec_out) return SFS2D_E_ARG;
  return read_last(pl, pl->div_out, out_host, cap, nrec_out, "sfs2d_plan_diversity");
}

// ------------------------------------------------------------------------------------------ window spectra

int sfs2d_plan_spectra(sfs2d_plan* pl, const int64_t* rec, const int32_t* grp, int64_t nsel, int64_t ngroups,
                       int64_t* out_dev) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  const sfs2d_window* recs = nullptr;
  int rc = post_ready(pl, "spectra", &recs);
  if (rc || (rc = sel_shape(pl, "spectra", rec, grp, nsel, ngroups))) return rc;
  pl->spec_sel_h.resize((size_t)nsel);
  int64_t nruns = 0, prev_g = -1;   // maximal runs of consecutive entries of one group
  rc = sel_walk(pl, "spectra", rec, grp, nsel, ngroups, false, [&](int64_t i, int64_t r, int64_t g) {
    pl->spec_sel_h[(size_t)i] = SpecSel{(uint32_t)r, (uint32_t)g};
    nruns += g != prev_g;
    prev_g = g;
    return 0;
  });
  if (rc) return rc;
  // groups x row in 64 bits: the row is at most 255 x 255 + 256 words
  const int64_t roww = (int64_t)pl->K.nb2 + pl->K.n1p + pl->K.n2p + 2;
  if ((rc = sel_rows_fit(pl, "spectra", ngroups, roww))) return rc;
  const int64_t words = ngroups * roww;
  hipStream_t st = CTX_STREAM(ctx);
  bool synced = false;
  int64_t* out = nullptr;
  if ((rc = reserve(ctx, st, pl->spec_sel, (size_t)nsel, &synced))) return rc;
  if ((rc = call_out(ctx, st, pl->spec_out, out_dev, (size_t)words, &synced, &out))) return rc;
  // the row's u32 histogram in LDS while a CU can hold it; above the default limit the family opts in, and a
  // refusal selects the global-atomic instantiations (as k_prep's histogram)
  const size_t lds = sizeof(uint32_t) * (size_t)roww;
  const bool ldsh = lds <= 160 * 1024 && (lds <= 64 * 1024 || grant_lds<SpecWin>(ctx, lds));
  HIPCHK(ctx, hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)words, st));
  pl->spec_out.last = out;
  pl->spec_out.n = words;
  if (nsel == 0) return 0;
  HIPCHK(ctx, hipMemcpyAsync(pl->spec_sel.p, pl->spec_sel_h.data(), sizeof(SpecSel) * (size_t)nsel, hipMemcpyHostToDevice, st));
  const SpecWin::Fn k = variant(ctx, SpecWin{pl->cnt, ldsh}, "k_spec_win", &rc);
  if (!k) return rc;
  // A contiguous run of the selection per workgroup, at most as many workgroups as are resident with the row in
  // LDS.  Every workgroup that holds entries of a group flushes into that group's row, and a workgroup walks its
  // entries one after another: 4,362 windows of ~358 SNPs pooled into one group took 50 us from 2,048 workgroups,
  // 38 us from 272 and 35 us from 1,090, against 23 us each in its own row.  So no more
  // workgroups than the selection has runs of one group -- but one per CU at least, and one per 4 entries, so that
  // a long pooled list is still streamed by the whole chip.
  const int per_cu = ldsh ? (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / lds)) : 8;
  const int64_t want = std::max<int64_t>(std::max<int64_t>(ctx->ncu, nruns), nsel / 4);
  const dim3 g((unsigned)std::min<int64_t>(nsel, std::min<int64_t>(want, (int64_t)per_cu * ctx->ncu)));
  hipLaunchKernelGGL(k, g, dim3(SPEC_BLOCK), ldsh ? lds : 0, st, pl->K, d->counts, scan_src(pl), recs, pl->spec_sel.p,
                     reinterpret_cast<unsigned long long*>(out), (uint32_t)nsel, (uint32_t)pl->nrec, (uint32_t)ngroups,
                     (uint32_t)d->n);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int sfs2d_plan_spectra_read(sfs2d_plan* pl, int64_t* out_host, int64_t cap_words, int64_t* nwords_out) {
  if (!pl || !nwords_out) return SFS2D_E_ARG;
  return read_last(pl, pl->spec_out, out_host, cap_words, nwords_out, "sfs2d_plan_spectra");
}

// ------------------------------------------------------------------------------------------ projected window spectra

namespace {
// ln k! for k < PROJ_LF: ascending sums of ln k in long double, rounded once (lf[0] = lf[1] = 0 exactly)
const double* proj_lf_table() {
  static const std::array<double, PROJ_LF> t = [] {
    std::array<double, PROJ_LF> a{};
    long double s = 0.0L;
    for (int k = 2; k < PROJ_LF; ++k) {
      s += std::log((long double)k);
      a[(size_t)k] = (double)s;
    }
    return a;
  }();
  return t.data();
}
}  // namespace

int sfs2d_project_weights(int32_t n, int32_t a, int32_t m, double* w_out) {
  if (!w_out || n < 0 || a < 0 || m < 0 || a > n || m > n || n >= PROJ_LF) return SFS2D_E_ARG;
  const double* lf = proj_lf_table();
  const double c = proj_lnc(lf, (uint32_t)n, (uint32_t)a, (uint32_t)m);
  for (int32_t j = 0; j <= m; ++j) w_out[j] = proj_w(lf, c, (uint32_t)n, (uint32_t)a, (uint32_t)m, (uint32_t)j);
  return 0;
}

namespace {

// the table of ln k! on the device, uploaded by the first call that projects
int proj_tables(sfs2d_ctx* ctx) {
  if (ctx->d_lf) return 0;
  const int rc = dalloc(ctx, &ctx->d_lf, (size_t)PROJ_LF);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpy(ctx->d_lf, proj_lf_table(), sizeof(double) * PROJ_LF, hipMemcpyHostToDevice));
  return 0;
}

// the fixed point 2^-e of a grid that receives B SNPs at most: e = min(40, 62 - bitlen(B))
int proj_fixed_point(unsigned __int128 B) {
  int b = 0;
  while (b < 64 && (B >> b) != 0) ++b;
  return std::min(40, 62 - b);
}

// k_proj_win over nsel selection entries into ngroups rows at the fixed point 2^-e (the rows zeroed by the caller)
int launch_proj_win(sfs2d_plan* pl, const sfs2d_window* recs, const ProjSel* sel, size_t nsel, unsigned long long* rows,
                    uint32_t ngroups, int32_t m1, int32_t m2, int e) {
  sfs2d_ctx* ctx = pl->ctx;
  // the row's u64 histogram in LDS while a CU can hold it beside the 4 KB table of ln k!; above the default limit
  // the family opts in, and a refusal selects the global-atomic instantiations
  const size_t lds = sizeof(unsigned long long) * ((size_t)(m1 + 1) * (size_t)(m2 + 1) + 2);
  const bool ldsh = lds + 4096 <= 160 * 1024 && (lds <= 64 * 1024 || grant_lds<ProjWin>(ctx, lds));
  int rc = 0;
  const ProjWin::Fn k = variant(ctx, ProjWin{pl->cnt, ldsh}, "k_proj_win", &rc);
  if (!k) return rc;
  // A contiguous run of the selection per workgroup, as many workgroups as are resident with the row in LDS (one
  // entry each at most).  Unlike k_spec_win the kernel is bound by its fp64 weights, not by the flushes: one
  // chromosome entry at (40, 40) of 50 took 790 us from 256 workgroups of 4,096-SNP pieces.
  const int per_cu = ldsh ? (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (lds + 4096))) : 8;
  const dim3 g((unsigned)std::min<int64_t>((int64_t)nsel, (int64_t)per_cu * ctx->ncu));
  hipLaunchKernelGGL(k, g, dim3(PROJ_BLOCK), ldsh ? lds : 0, CTX_STREAM(ctx), pl->K, pl->data->counts, scan_src(pl), recs, sel,
                     ctx->d_lf, rows, (uint32_t)nsel, (uint32_t)pl->nrec, ngroups, (uint32_t)pl->data->n, (uint32_t)m1,
                     (uint32_t)m2, std::ldexp(1.0, e), 1ull << (62 - e));
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// one chromosome as selection entries of group g: pieces of PROJ_CHUNK SNPs, consecutive entries of one group (a
// chromosome is streamed by many workgroups, where a record's range is known on the device alone); returns its SNPs
int64_t push_chrom(std::vector<ProjSel>& sel, const sfs2d_data* d, int64_t c, uint32_t g) {
  const int64_t cb = d->chrom_off[(size_t)c], ce = d->chrom_off[(size_t)c + 1];
  for (int64_t s = cb; s < ce; s += PROJ_CHUNK)
    sel.push_back(ProjSel{0xffffffffu, g, (uint32_t)s, (uint32_t)std::min<int64_t>(s + PROJ_CHUNK, ce)});
  return ce - cb;
}

}  // namespace

int sfs2d_plan_project(sfs2d_plan* pl, int32_t m1, int32_t m2, const int64_t* rec, const int32_t* grp, int64_t nsel,
                       int64_t ngroups, int64_t* out_dev, int32_t* e_out) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  const sfs2d_window* recs = nullptr;
  int rc = post_ready(pl, "project", &recs);
  if (rc) return rc;
  if (m1 < 2 || m1 > pl->K.n1 || m2 < 2 || m2 > pl->K.n2)
    return set_err(ctx, SFS2D_E_ARG, "project: (m1, m2) = (" + std::to_string(m1) + ", " + std::to_string(m2) +
                                         ") outside [2, " + std::to_string(pl->K.n1) + "] x [2, " + std::to_string(pl->K.n2) + "]");
  const int64_t roww = (int64_t)(m1 + 1) * (m2 + 1) + 2;   // at most 255 x 255 + 2 words
  if ((rc = sel_shape(pl, "project", rec, grp, nsel, ngroups)) || (rc = sel_rows_fit(pl, "project", ngroups, roww))) return rc;
  pl->proj_sel_h.clear();
  pl->proj_sel_h.reserve((size_t)nsel);
  // B: the SNPs one group can receive -- its entries times the bound on one entry's SNPs (a record's: plan_create's
  // maxsnp; with chromosome entries in the selection, the longest chromosome, which is no smaller)
  int64_t per_entry = std::max<int64_t>(1, pl->maxsnp);
  rc = sel_walk(pl, "project", rec, grp, nsel, ngroups, true, [&](int64_t i, int64_t r, int64_t g) {
    if (r >= 0) {
      pl->proj_sel_h.push_back(ProjSel{(uint32_t)r, (uint32_t)g, 0u, 0u});
      return 0;
    }
    const int64_t c = -(r + 1);   // -(c + 1): the whole chromosome c
    if (c >= d->nchrom)
      return set_err(ctx, SFS2D_E_ARG, "project: entry " + std::to_string(i) + ": chromosome " + std::to_string(c) +
                                           " outside [0, " + std::to_string(d->nchrom) + ")");
    per_entry = std::max<int64_t>(per_entry, push_chrom(pl->proj_sel_h, d, c, (uint32_t)g));
    return 0;
  });
  if (rc) return rc;
  int64_t maxent = nsel ? 1 : 0;   // the most entries of one group (grp == NULL: one each)
  if (grp) {
    std::vector<int32_t> gs(grp, grp + nsel);
    std::sort(gs.begin(), gs.end());
    for (int64_t i = 0, run = 0; i < nsel; ++i) {
      run = (i && gs[(size_t)i] == gs[(size_t)i - 1]) ? run + 1 : 1;
      maxent = std::max(maxent, run);
    }
  }
  const int e = proj_fixed_point((unsigned __int128)std::max<int64_t>(1, maxent) * (unsigned __int128)per_entry);
  if (e < 8)
    return set_err(ctx, SFS2D_E_CAP, "project: " + std::to_string(maxent) + " entries of up to " + std::to_string(per_entry) +
                                         " SNPs in one group leave fewer than 8 fraction bits in 64-bit sums");
  if (e_out) *e_out = e;
  nsel = (int64_t)pl->proj_sel_h.size();   // (from here on: the entries the kernel walks)
  if (nsel > 0xffffffffll) return set_err(ctx, SFS2D_E_ARG, "project: more than 2^32 - 1 selection entries");
  const int64_t words = ngroups * roww;
  hipStream_t st = CTX_STREAM(ctx);
  if ((rc = proj_tables(ctx))) return rc;
  bool synced = false;
  int64_t* out = nullptr;
  if ((rc = reserve(ctx, st, pl->proj_sel, (size_t)nsel, &synced))) return rc;
  if ((rc = call_out(ctx, st, pl->proj_out, out_dev, (size_t)words, &synced, &out))) return rc;   // (words; n: groups)
  HIPCHK(ctx, hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)words, st));
  pl->proj_out.last = out;
  pl->proj_out.n = ngroups;
  pl->proj_roww = roww;
  pl->proj_e = e;
  if (nsel == 0) return 0;
  HIPCHK(ctx, hipMemcpyAsync(pl->proj_sel.p, pl->proj_sel_h.data(), sizeof(ProjSel) * (size_t)nsel, hipMemcpyHostToDevice, st));
  return launch_proj_win(pl, recs, pl->proj_sel.p, (size_t)nsel, reinterpret_cast<unsigned long long*>(out), (uint32_t)ngroups,
                         m1, m2, e);
}

int sfs2d_plan_project_read(sfs2d_plan* pl, double* out_host, int64_t* used, int64_t* dropped, int64_t cap_groups,
                            int64_t* ngroups_out, int64_t* words_per_group) {
  if (!pl || !ngroups_out || !words_per_group) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  if (pl->proj_out.n >= 0) *words_per_group = pl->proj_roww - 2;
  const int rc = read_ready(pl, pl->proj_out, cap_groups, ngroups_out, "sfs2d_plan_project");
  if (rc) return rc;
  if (!out_host || !used || !dropped) return SFS2D_E_ARG;
  const size_t roww = (size_t)pl->proj_roww, ngrid = roww - 2, ng = (size_t)pl->proj_out.n;
  std::vector<int64_t> raw;
  try {
    raw.resize(ng * roww);
  } catch (const std::bad_alloc&) {
    return set_err(ctx, SFS2D_E_NOMEM, "project_read: host staging buffer");
  }
  HIPCHK(ctx, hipMemcpyAsync(raw.data(), pl->proj_out.last, sizeof(int64_t) * raw.size(), hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  const double inv = std::ldexp(1.0, -pl->proj_e);
  for (size_t g = 0; g < ng; ++g) {
    const int64_t* r = raw.data() + g * roww;
    for (size_t k = 0; k < ngrid; ++k) out_host[g * ngrid + k] = (double)r[k] * inv;
    used[g] = r[ngrid];
    dropped[g] = r[ngrid + 1];
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ projected scan

namespace {

// The fixed points of a projected scan of this plan, shared by sfs2d_plan_project_scan and sfs2d_plan_project_null so
// that observed and null values carry the same rounding -- windows: one record per grid; backgrounds: one chromosome
// entry per row (section 18's rule for such a call) -- and the background chromosomes' selection (bg_chrom < 0:
// every chromosome, group = chromosome; else that one, group 0).  SFS2D_E_CAP below 8 fraction bits.
int pscan_fixed_points(sfs2d_plan* pl, const char* name, int32_t bg_chrom, std::vector<ProjSel>& sel, int* e_out,
                       int* e_bg_out) {
  const sfs2d_data* d = pl->data;
  const int64_t per_rec = std::max<int64_t>(1, pl->maxsnp);
  const int nbg = bg_chrom < 0 ? d->nchrom : 1;
  int64_t per_bg = per_rec;
  sel.clear();
  for (int g = 0; g < nbg; ++g) per_bg = std::max<int64_t>(per_bg, push_chrom(sel, d, bg_chrom < 0 ? g : bg_chrom, (uint32_t)g));
  const int e = proj_fixed_point((unsigned __int128)per_rec), e_bg = proj_fixed_point((unsigned __int128)per_bg);
  if (e < 8 || e_bg < 8)
    return set_err(pl->ctx, SFS2D_E_CAP, std::string(name) + ": up to " + std::to_string(e < 8 ? per_rec : per_bg) +
                                             " SNPs in one grid leave fewer than 8 fraction bits in 64-bit sums");
  *e_out = e;
  *e_bg_out = e_bg;
  return 0;
}

}  // namespace

int sfs2d_plan_project_scan(sfs2d_plan* pl, int32_t m1, int32_t m2, int32_t bg_chrom, sfs2d_projstat* out_dev,
                            int32_t* e_out, int32_t* e_bg_out) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  const sfs2d_window* recs = nullptr;
  int rc = post_ready(pl, "project_scan", &recs);
  if (rc) return rc;
  if (pl->prm.bg_mode == SFS2D_BG_SUPPLIED)
    return set_err(ctx, SFS2D_E_ARG, "project_scan: a plan with a supplied background has no projected background "
                                     "(only per-chromosome plans; bg_chrom names one chromosome for every record)");
  if (m1 < 2 || m1 > pl->K.n1 || m2 < 2 || m2 > pl->K.n2)
    return set_err(ctx, SFS2D_E_ARG, "project_scan: (m1, m2) = (" + std::to_string(m1) + ", " + std::to_string(m2) +
                                         ") outside [2, " + std::to_string(pl->K.n1) + "] x [2, " + std::to_string(pl->K.n2) + "]");
  if (bg_chrom < -1 || bg_chrom >= d->nchrom)
    return set_err(ctx, SFS2D_E_ARG, "project_scan: bg_chrom " + std::to_string(bg_chrom) + " outside [-1, " +
                                         std::to_string(d->nchrom) + ")");
  if (pl->nrec > 0xffffffffll) return set_err(ctx, SFS2D_E_ARG, "project_scan: more than 2^32 - 1 records");
  const int64_t ngrid = (int64_t)(m1 + 1) * (m2 + 1), roww = ngrid + 2, lpw = ngrid + (m1 + 1) + (m2 + 1);
  // the window grid, its marginals and sums in LDS beside the 4 KB table: there is no global-memory variant (a
  // grid per window in HBM is what this call avoids)
  const size_t lds = sizeof(unsigned long long) * pscan_lds_words((uint32_t)m1, (uint32_t)m2);
  if (lds + 4096 > 160 * 1024)
    return set_err(ctx, SFS2D_E_CAP, "project_scan: the (" + std::to_string(m1 + 1) + " x " + std::to_string(m2 + 1) +
                                         ") window grid takes " + std::to_string(lds + 4096) +
                                         " bytes of LDS, more than the 163840 of a compute unit");
  const int nbg = bg_chrom < 0 ? d->nchrom : 1;
  int e = 0, e_bg = 0;
  if ((rc = pscan_fixed_points(pl, "project_scan", bg_chrom, pl->pscan_sel_h, &e, &e_bg))) return rc;
  if (e_out) *e_out = e;
  if (e_bg_out) *e_bg_out = e_bg;
  const size_t nsel = pl->pscan_sel_h.size();
  if (nsel > 0xffffffffull) return set_err(ctx, SFS2D_E_ARG, "project_scan: more than 2^32 - 1 background pieces");
  hipStream_t st = CTX_STREAM(ctx);
  if ((rc = proj_tables(ctx))) return rc;
  const size_t bgw = (size_t)nbg * (size_t)roww, lpn = (size_t)nbg * (size_t)lpw;
  bool synced = false;
  sfs2d_projstat* out = nullptr;
  if ((rc = reserve(ctx, st, pl->pscan_sel, nsel, &synced)) || (rc = reserve(ctx, st, pl->pscan_bg, bgw, &synced)) ||
      (rc = reserve(ctx, st, pl->pscan_lp, lpn, &synced)) ||
      (rc = call_out(ctx, st, pl->pscan_out, out_dev, (size_t)pl->nrec, &synced, &out)))
    return rc;
  // above the default limit the family opts in
  if (lds + 4096 > 64 * 1024 && !grant_lds<ProjScan>(ctx, lds))
    return set_err(ctx, SFS2D_E_CAP, "project_scan: the device refuses " + std::to_string(lds) +
                                         " bytes of dynamic LDS for k_proj_scan");
  const ProjScan::Fn ks = variant(ctx, ProjScan{pl->cnt}, "k_proj_scan", &rc);
  if (!ks) return rc;
  pl->pscan_out.last = out;
  pl->pscan_out.n = pl->nrec;
  if (pl->nrec == 0) return 0;
  // the background chromosomes' rows by k_proj_win (chromosome entries, as sfs2d_plan_project launches them) ...
  HIPCHK(ctx, hipMemsetAsync(pl->pscan_bg.p, 0, sizeof(unsigned long long) * bgw, st));
  if (nsel) {
    HIPCHK(ctx, hipMemcpyAsync(pl->pscan_sel.p, pl->pscan_sel_h.data(), sizeof(ProjSel) * nsel, hipMemcpyHostToDevice, st));
    if ((rc = launch_proj_win(pl, recs, pl->pscan_sel.p, nsel, pl->pscan_bg.p, (uint32_t)nbg, m1, m2, e_bg))) return rc;
  }
  // ... their ln tables, and every record against its chromosome's
  hipLaunchKernelGGL(k_proj_lp, dim3((unsigned)nbg), dim3(PROJ_BLOCK), 0, st, pl->pscan_bg.p, pl->pscan_lp.p, (uint32_t)m1,
                     (uint32_t)m2, pl->K.fold);
  HIPCHK(ctx, hipGetLastError());
  const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (lds + 4096)));
  const dim3 g((unsigned)std::min<int64_t>(pl->nrec, (int64_t)per_cu * ctx->ncu));
  hipLaunchKernelGGL(ks, g, dim3(PROJ_BLOCK), lds, st, pl->K, d->counts, scan_src(pl), recs, ctx->d_lf, pl->pscan_lp.p, out,
                     (uint32_t)pl->nrec, (uint32_t)nbg, (uint32_t)d->n, (uint32_t)m1, (uint32_t)m2, bg_chrom < 0 ? 0 : 1,
                     std::ldexp(1.0, e), std::ldexp(1.0, -e), (uint32_t)e);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int sfs2d_plan_project_scan_read(sfs2d_plan* pl, sfs2d_projstat* out_host, int64_t cap, int64_t* nrec_out) {
  if (!pl || !nrec_out) return SFS2D_E_ARG;
  return read_last(pl, pl->pscan_out, out_host, cap, nrec_out, "sfs2d_plan_project_scan");
}

// ------------------------------------------------------------------------------------------ projected null

namespace {

// The pools of (the plan's last executed run, m1, m2): pool_idx -- every SNP index sorted by its stratum cell
// (chromosome, n1c - m1, n2c - m2), stable, so ascending within a stratum, the SNPs in no pool last -- and the dense
// table of (start, size) per cell; beside them the background chromosomes' rows and ln tables at e_bg.  Built by the
// first call after a run or with another projection and kept on the plan.  Set-up, not the hot path: the sort is
// rocprim's stable radix sort over the cell index's bits; its key and value arrays are freed when it is done.
int pnull_pools(sfs2d_plan* pl, const sfs2d_window* recs, int32_t m1, int32_t m2, int e_bg, bool* synced) {
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  if (pl->pnull_done == pl->done && pl->pnull_m1 == m1 && pl->pnull_m2 == m2) return 0;
  pl->pnull_done = 0;
  hipStream_t st = CTX_STREAM(ctx);
  const uint32_t n = (uint32_t)d->n, nchrom = (uint32_t)d->nchrom;
  // u8 counts: a called count is at most 510, whatever the data set reports (wrapped device data: nothing)
  const uint32_t mx1 = std::max<uint32_t>((uint32_t)m1, std::min<uint32_t>(510u, d->max_nc1));
  const uint32_t mx2 = std::max<uint32_t>((uint32_t)m2, std::min<uint32_t>(510u, d->max_nc2));
  const PnullDims D{mx1 - (uint32_t)m1 + 1u, mx2 - (uint32_t)m2 + 1u};
  const unsigned long long ncell = (unsigned long long)nchrom * D.d1 * D.d2;
  if (ncell >= 0xffffffffull)
    return set_err(ctx, SFS2D_E_CAP, "project_null: " + std::to_string(nchrom) + " chromosomes x " + std::to_string(D.d1) +
                                         " x " + std::to_string(D.d2) + " called-count pairs do not fit a 32-bit stratum index");
  int rc = 0;
  const int64_t ngrid = (int64_t)(m1 + 1) * (m2 + 1), roww = ngrid + 2, lpw = ngrid + (m1 + 1) + (m2 + 1);
  const size_t nsel = pl->pnull_bgsel_h.size(), bgw = (size_t)nchrom * (size_t)roww, lpn = (size_t)nchrom * (size_t)lpw;
  if ((rc = reserve(ctx, st, pl->pnull_pool, (size_t)n, synced)) || (rc = reserve(ctx, st, pl->pnull_tab, (size_t)ncell, synced)) ||
      (rc = reserve(ctx, st, pl->pnull_bgsel, nsel, synced)) || (rc = reserve(ctx, st, pl->pnull_bg, bgw, synced)) ||
      (rc = reserve(ctx, st, pl->pnull_lp, lpn, synced)))
    return rc;
  // the backgrounds, as sfs2d_plan_project_scan builds them
  HIPCHK(ctx, hipMemsetAsync(pl->pnull_bg.p, 0, sizeof(unsigned long long) * bgw, st));
  if (nsel) {
    HIPCHK(ctx, hipMemcpyAsync(pl->pnull_bgsel.p, pl->pnull_bgsel_h.data(), sizeof(ProjSel) * nsel, hipMemcpyHostToDevice, st));
    if ((rc = launch_proj_win(pl, recs, pl->pnull_bgsel.p, nsel, pl->pnull_bg.p, nchrom, m1, m2, e_bg))) return rc;
  }
  hipLaunchKernelGGL(k_proj_lp, dim3(nchrom), dim3(PROJ_BLOCK), 0, st, pl->pnull_bg.p, pl->pnull_lp.p, (uint32_t)m1,
                     (uint32_t)m2, pl->K.fold);
  HIPCHK(ctx, hipGetLastError());
  // the pools
  uint32_t *key_in = nullptr, *key_out = nullptr, *val_in = nullptr;
  void* tmp = nullptr;
  auto done = [&](int code) {
    hipFree(key_in); hipFree(key_out); hipFree(val_in); hipFree(tmp);   // (hipFree waits for the device)
    return code;
  };
  if ((rc = dalloc(ctx, &key_in, (size_t)n)) || (rc = dalloc(ctx, &key_out, (size_t)n)) || (rc = dalloc(ctx, &val_in, (size_t)n)))
    return done(rc);
  const dim3 gk((n + 255u) / 256u);
  if (pl->cnt)
    hipLaunchKernelGGL(k_pnull_keys<true>, gk, dim3(256), 0, st, pl->K, d->counts, scan_src(pl), d->d_chrom_off, nchrom, n,
                       (uint32_t)m1, (uint32_t)m2, D, (uint32_t)ncell, key_in, val_in);
  else
    hipLaunchKernelGGL(k_pnull_keys<false>, gk, dim3(256), 0, st, pl->K, d->counts, scan_src(pl), d->d_chrom_off, nchrom, n,
                       (uint32_t)m1, (uint32_t)m2, D, (uint32_t)ncell, key_in, val_in);
  if (hipGetLastError() != hipSuccess) return done(set_err(ctx, SFS2D_E_HIP, "project_null: k_pnull_keys launch"));
  size_t tmp_bytes = 0;
  // (the key of a SNP in no pool is ncell and sorts last: the bits of ncell are all the sort reads)
  unsigned bits = 1;
  while (bits < 32 && (ncell >> bits) != 0) ++bits;
  if (rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_in, key_out, val_in, pl->pnull_pool.p, (size_t)n, 0u, bits, st) != hipSuccess)
    return done(set_err(ctx, SFS2D_E_HIP, "project_null: radix sort (size query)"));
  if (hipMalloc(&tmp, std::max<size_t>(tmp_bytes, 1)) != hipSuccess) {
    (void)hipGetLastError();
    return done(set_err(ctx, SFS2D_E_NOMEM, "project_null: radix sort workspace"));
  }
  if (rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, val_in, pl->pnull_pool.p, (size_t)n, 0u, bits, st) != hipSuccess)
    return done(set_err(ctx, SFS2D_E_HIP, "project_null: radix sort"));
  if (hipMemsetAsync(pl->pnull_tab.p, 0, sizeof(uint2) * (size_t)std::max<unsigned long long>(1, ncell), st) != hipSuccess)
    return done(set_err(ctx, SFS2D_E_HIP, "project_null: stratum table memset"));
  for (int phase = 0; phase < 2; ++phase)
    hipLaunchKernelGGL(k_pnull_heads, gk, dim3(256), 0, st, key_out, n, (uint32_t)ncell, pl->pnull_tab.p, phase);
  if (hipGetLastError() != hipSuccess) return done(set_err(ctx, SFS2D_E_HIP, "project_null: k_pnull_heads launch"));
  if (hipStreamSynchronize(st) != hipSuccess) return done(set_err(ctx, SFS2D_E_HIP, "project_null: pool build"));
  done(0);
  pl->pnull_done = pl->done;
  pl->pnull_m1 = m1;
  pl->pnull_m2 = m2;
  pl->pnull_dims = D;
  return 0;
}

}  // namespace

int sfs2d_plan_project_null(sfs2d_plan* pl, int32_t m1, int32_t m2, const sfs2d_null_params* np, const int64_t* rec,
                            int64_t nsel, sfs2d_projstat* out_dev, uint32_t* thin_dev, int32_t* e_out, int32_t* e_bg_out) {
  if (!pl) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  const sfs2d_data* d = pl->data;
  if (!np) return set_err(ctx, SFS2D_E_ARG, "project_null: null argument");
  const sfs2d_window* recs = nullptr;
  int rc = post_ready(pl, "project_null", &recs);
  if (rc) return rc;
  if (pl->prm.bg_mode == SFS2D_BG_SUPPLIED)
    return set_err(ctx, SFS2D_E_ARG, "project_null: a plan with a supplied background has no projected background "
                                     "(only per-chromosome plans)");
  if (m1 < 2 || m1 > pl->K.n1 || m2 < 2 || m2 > pl->K.n2)
    return set_err(ctx, SFS2D_E_ARG, "project_null: (m1, m2) = (" + std::to_string(m1) + ", " + std::to_string(m2) +
                                         ") outside [2, " + std::to_string(pl->K.n1) + "] x [2, " + std::to_string(pl->K.n2) + "]");
  if (np->replicates < 1) return set_err(ctx, SFS2D_E_ARG, "project_null: replicates must be >= 1");
  if (pl->nrec > 0xffffffffll) return set_err(ctx, SFS2D_E_ARG, "project_null: more than 2^32 - 1 records");
  if (nsel < 0) return set_err(ctx, SFS2D_E_ARG, "project_null: nsel must be >= 0");
  if (!rec && nsel != pl->nrec)
    return set_err(ctx, SFS2D_E_ARG, "project_null: rec == NULL selects every record in order: nsel must be the plan's record count");
  pl->pnull_sel_h.resize(rec ? (size_t)nsel : 0);
  for (int64_t i = 0; rec && i < nsel; ++i) {
    if (rec[i] < 0 || rec[i] >= pl->nrec)
      return set_err(ctx, SFS2D_E_ARG, "project_null: entry " + std::to_string(i) + ": record " + std::to_string(rec[i]) +
                                           " outside [0, " + std::to_string(pl->nrec) + ")");
    pl->pnull_sel_h[(size_t)i] = (uint32_t)rec[i];
  }
  const unsigned long long nout = (unsigned long long)nsel * np->replicates;
  if (nout > (1ull << 26))
    return set_err(ctx, SFS2D_E_CAP, "project_null: more than 2^26 records in one call (split the selection)");
  const size_t lds = sizeof(unsigned long long) * pscan_lds_words((uint32_t)m1, (uint32_t)m2);
  if (lds + 4096 > 160 * 1024)
    return set_err(ctx, SFS2D_E_CAP, "project_null: the (" + std::to_string(m1 + 1) + " x " + std::to_string(m2 + 1) +
                                         ") window grid takes " + std::to_string(lds + 4096) +
                                         " bytes of LDS, more than the 163840 of a compute unit");
  int e = 0, e_bg = 0;
  if ((rc = pscan_fixed_points(pl, "project_null", -1, pl->pnull_bgsel_h, &e, &e_bg))) return rc;
  if (e_out) *e_out = e;
  if (e_bg_out) *e_bg_out = e_bg;
  hipStream_t st = CTX_STREAM(ctx);
  if ((rc = proj_tables(ctx))) return rc;
  bool synced = false;
  sfs2d_projstat* out = nullptr;
  uint32_t* thin = nullptr;
  if ((rc = reserve(ctx, st, pl->pnull_sel, pl->pnull_sel_h.size(), &synced)) ||
      (rc = call_out(ctx, st, pl->pnull_out, out_dev, (size_t)nout, &synced, &out)) ||
      (rc = call_out(ctx, st, pl->pnull_thin, thin_dev, (size_t)nsel, &synced, &thin)))
    return rc;
  if (lds + 4096 > 64 * 1024 && !grant_lds<ProjNull>(ctx, lds))
    return set_err(ctx, SFS2D_E_CAP, "project_null: the device refuses " + std::to_string(lds) +
                                         " bytes of dynamic LDS for k_proj_null");
  const ProjNull::Fn kn = variant(ctx, ProjNull{pl->cnt}, "k_proj_null", &rc);
  if (!kn) return rc;
  if (nout && (rc = pnull_pools(pl, recs, m1, m2, e_bg, &synced))) {
    pl->pnull_out.last = nullptr; pl->pnull_out.n = -1;
    pl->pnull_thin.last = nullptr; pl->pnull_thin.n = -1;
    return rc;
  }
  pl->pnull_out.last = out;
  pl->pnull_out.n = (int64_t)nout;
  pl->pnull_thin.last = thin;
  pl->pnull_thin.n = nsel;
  if (nout == 0) return 0;
  if (rec)
    HIPCHK(ctx, hipMemcpyAsync(pl->pnull_sel.p, pl->pnull_sel_h.data(), sizeof(uint32_t) * (size_t)nsel, hipMemcpyHostToDevice, st));
  const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / (lds + 4096)));
  const dim3 g((unsigned)std::min<unsigned long long>(nout, (unsigned long long)per_cu * ctx->ncu));
  const uint2 key = make_uint2((uint32_t)np->seed, (uint32_t)(np->seed >> 32));
  hipLaunchKernelGGL(kn, g, dim3(PROJ_BLOCK), lds, st, pl->K, d->counts, scan_src(pl), recs, rec ? pl->pnull_sel.p : nullptr,
                     ctx->d_lf, pl->pnull_lp.p, pl->pnull_tab.p, pl->pnull_pool.p, out, thin, (uint32_t)nout, np->replicates, key,
                     (uint32_t)d->nchrom, (uint32_t)d->n, (uint32_t)m1, (uint32_t)m2, pl->pnull_dims, std::ldexp(1.0, e),
                     std::ldexp(1.0, -e), (uint32_t)e);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int sfs2d_plan_project_null_read(sfs2d_plan* pl, sfs2d_projstat* out_host, uint32_t* thin_host, int64_t cap, int64_t* nrec_out) {
  if (!pl || !nrec_out) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  // (out_host NULL: the records are not wanted -- they may be in the caller's device buffer -- and cap is not read)
  const int rc = read_ready(pl, pl->pnull_out, out_host ? cap : INT64_MAX, nrec_out, "sfs2d_plan_project_null");
  if (rc) return rc;
  if (pl->pnull_thin.n > 0 && thin_host)
    HIPCHK(ctx, hipMemcpyAsync(thin_host, pl->pnull_thin.last, sizeof(uint32_t) * (size_t)pl->pnull_thin.n, hipMemcpyDeviceToHost,
                               CTX_STREAM(ctx)));
  if (pl->pnull_out.n > 0 && out_host)
    HIPCHK(ctx, hipMemcpyAsync(out_host, pl->pnull_out.last, sizeof(sfs2d_projstat) * (size_t)pl->pnull_out.n,
                               hipMemcpyDeviceToHost, CTX_STREAM(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(CTX_STREAM(ctx)));
  return 0;
}

int sfs2d_plan_time(sfs2d_plan* pl, int iters, double* ms_run, double* ms_k1, double* ms_k2, double* ms_k3) {
  if (!pl || iters < 1) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = pl->ctx;
  hipStream_t st = CTX_STREAM(ctx);
  double t1 = 0, t2 = 0, t3 = 0, tall = 0;
  int rc = 0;
  for (int it = 0; it < iters; ++it) {
    HIPCHK(ctx, hipEventRecord(pl->ev[0], st));
    if (pl->seg_index) HIPCHK(ctx, stage_slots(pl));
    if (slots_only(pl)) HIPCHK(ctx, launch_slots_only(pl));
    else if ((rc = launch_prep(pl, true))) return rc;
    if (free_slots(pl)) HIPCHK(ctx, launch_slots_slide(pl, false));
    HIPCHK(ctx, hipEventRecord(pl->ev[1], st));
    if (pl->do_bg && !pl->fused) HIPCHK(ctx, launch_bg_slices(pl));
    if (free_slots(pl) && pl->fst_win) HIPCHK(ctx, launch_fst_win(pl));
    for (sfs2d_plan* a : pl->attached)
      if ((rc = launch_attached(a))) return rc;
    HIPCHK(ctx, hipEventRecord(pl->ev[2], st));
    if ((rc = launch_scan_any(pl, pl->d_out))) return rc;
    pl->runs++;
    pl->done++;
    HIPCHK(ctx, hipEventRecord(pl->ev[3], st));
    HIPCHK(ctx, hipEventSynchronize(pl->ev[3]));
    float a = 0, b = 0, c = 0, d = 0;
    hipEventElapsedTime(&a, pl->ev[0], pl->ev[1]);
    hipEventElapsedTime(&b, pl->ev[1], pl->ev[2]);
    hipEventElapsedTime(&c, pl->ev[2], pl->ev[3]);
    hipEventElapsedTime(&d, pl->ev[0], pl->ev[3]);
    t1 += a; t2 += b; t3 += c; tall += d;
  }
  pl->last_out = pl->d_out;
  if (ms_run) *ms_run = tall / iters;
  if (ms_k1) *ms_k1 = t1 / iters;
  if (ms_k2) *ms_k2 = t2 / iters;
  if (ms_k3) *ms_k3 = t3 / iters;
  return 0;
}

int sfs2d_plan_destroy(sfs2d_plan* pl) {
  if (!pl) return SFS2D_E_ARG;
  hipSetDevice(pl->ctx->device);
  hipStreamSynchronize(CTX_STREAM(pl->ctx));
  for (sfs2d_plan* a : pl->attached) {   // attached plans go with their base
    a->base = pl;
    plan_free(a);
    delete a;
  }
  pl->attached.clear();
  if (pl->base) {
    auto& v = pl->base->attached;
    v.erase(std::remove(v.begin(), v.end(), pl), v.end());
  }
  plan_free(pl);
  delete pl;
  return 0;
}

static int plan_attach(sfs2d_plan* base, const sfs2d_params* prm, int64_t step, const RegionList* rg, sfs2d_plan** out);

int sfs2d_plan_attach(sfs2d_plan* base, const sfs2d_params* prm, sfs2d_plan** out) {
  return plan_attach(base, prm, 0, nullptr, out);
}

// a regions plan attached to an ordinary, sliding or regions base: the rules of an attached sliding plan
int sfs2d_plan_attach_regions(sfs2d_plan* base, const sfs2d_params* prm, const int32_t* chrom, const uint32_t* first,
                              const uint32_t* last, int64_t n, sfs2d_plan** out) {
  if (!base || !prm || !out) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = base->ctx;
  *out = nullptr;
  KParams K;
  int rc = make_kparams(ctx, prm, base->data->nchrom, &K);
  const RegionList rg{chrom, first, last, n};
  sfs2d_params p = *prm;
  if (!rc) rc = check_regions(ctx, prm, base->data->nchrom, rg, &p.window);
  return rc ? rc : plan_attach(base, &p, 0, &rg, out);
}

int sfs2d_plan_attach_sliding(sfs2d_plan* base, const sfs2d_params* prm, int64_t step, sfs2d_plan** out) {
  if (!base || !prm || !out) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = base->ctx;
  *out = nullptr;
  KParams K;
  int rc = make_kparams(ctx, prm, base->data->nchrom, &K);
  if (!rc) rc = check_step(ctx, prm, step);
  if (rc) return rc;
  // step == window is the disjoint geometry: the ordinary attached plan (byte-equal by construction), unless
  // it is refused for its Fst rule alone -- a sliding plan's Fst needs no sums of the base
  if (step == prm->window && plan_attach(base, prm, 0, nullptr, out) == 0) return 0;
  return plan_attach(base, prm, step, nullptr, out);
}

// step: 0 an ordinary attached plan; > 0 a sliding one (checked by check_step); rg: a regions one (check_regions)
static int plan_attach(sfs2d_plan* base, const sfs2d_params* prm, int64_t step, const RegionList* rg, sfs2d_plan** out) {
  if (!base || !prm || !out) return SFS2D_E_ARG;
  sfs2d_ctx* ctx = base->ctx;
  *out = nullptr;
  if (base->base) return set_err(ctx, SFS2D_E_ARG, "attach to a base plan, not to an attached one");
  const bool large = base->do_bg && base->G != WAVE;   // tables from the base's k_bg_slice (with its tail)
  if (!base->fused && !base->sliced && !large)
    return set_err(ctx, SFS2D_E_ARG, "attached plans need a per-chromosome-background base plan");
  const sfs2d_params& b = base->prm;
  if (prm->n1p != b.n1p || prm->n2p != b.n2p || (prm->fold != 0) != (b.fold != 0) || prm->bg_mode != b.bg_mode ||
      prm->ann_want != b.ann_want || prm->has_start != b.has_start || prm->has_end != b.has_end ||
      (prm->has_start && prm->start_pos != b.start_pos) || (prm->has_end && prm->end_pos != b.end_pos))
    return set_err(ctx, SFS2D_E_ARG, "an attached plan may differ from its base only in the window and flags");
  const bool bp = prm->window_mode == SFS2D_WINDOW_BP;
  sfs2d_plan* a = nullptr;
  int rc = plan_create(ctx, base->data, prm, base->sliced ? 1 : 0, step, rg, &a);
  if (rc) return rc;
  if (a->fused != base->fused || a->sliced != base->sliced || a->G != base->G || a->cnt != base->cnt) {
    plan_free(a); delete a;
    return set_err(ctx, SFS2D_E_ARG, "attached plan would take a different kernel path than its base");
  }
  // Fst of an attached plan: its own scan's sums (fst_scan), else the base's k_prep sums added per
  // attached window (fused bases) or k_fst_win on the attached slots (sliced bases)
  uint32_t m = 0;
  // (a sliding or regions attached plan: its own k_fst_win, whatever the base; a sliding or regions base has no
  // k_prep sums to add)
  if ((prm->flags & SFS2D_F_FST) && !a->fst_scan && !step && !rg) {
    const bool base_bp = b.window_mode == SFS2D_WINDOW_BP;
    const char* why = nullptr;
    if (!bp) why = "attached Fst needs fixed-bp windows";
    else if (!base->sliced && (!(b.flags & SFS2D_F_FST) || base->fst_scan || base->fst_win || !base_bp || prm->window % b.window != 0))
      why = "attached Fst needs a fixed-bp Fst base plan whose window divides this one's";
    if (why) { plan_free(a); delete a; return set_err(ctx, SFS2D_E_ARG, why); }
    if (!base->sliced) m = (uint32_t)(prm->window / b.window);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipFree(a->d_bins); hipFree(a->d_repl); hipFree(a->d_bcount);
  a->d_bins = base->d_bins;
  a->d_repl = base->d_repl;
  a->d_bcount = base->d_bcount;
  if (base->sliced) {   // the base's k_bg_slice tables (the attached scans combine the same leaf sums)
    hipFree(a->d_tab); hipFree(a->d_lp); hipFree(a->d_head); hipFree(a->d_leafsum); hipFree(a->d_bg1d);
    a->d_tab = base->d_tab;
    a->d_lp = base->d_lp;
    a->d_head = base->d_head;
    a->d_leafsum = base->d_leafsum;
    a->d_bg1d = base->d_bg1d;
  } else if (large) {   // the base's finished per-chromosome tables
    hipFree(a->d_tab); hipFree(a->d_lp); hipFree(a->d_head);
    a->d_tab = base->d_tab;
    a->d_lp = base->d_lp;
    a->d_head = base->d_head;
  }
  a->base = base;
  a->fst_m = m;
  a->fst_win = (base->sliced || step || rg) && (prm->flags & SFS2D_F_FST) && !a->fst_scan;   // k_fst_win on the attached slots
  a->nfst = 0;
  rc = 0;
  std::vector<uint32_t> sb(a->slot_base_h.begin(), a->slot_base_h.end());
  if (!a->d_slot_base) rc = rc ? rc : dalloc(ctx, &a->d_slot_base, sb.size());
  if (m && !base->d_slot_base) {
    std::vector<uint32_t> bsb(base->slot_base_h.begin(), base->slot_base_h.end());
    rc = rc ? rc : dalloc(ctx, &base->d_slot_base, bsb.size());
    if (!rc && hipMemcpy(base->d_slot_base, bsb.data(), sizeof(uint32_t) * bsb.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = SFS2D_E_HIP;
  }
  if (!rc && hipMemcpy(a->d_slot_base, sb.data(), sizeof(uint32_t) * sb.size(), hipMemcpyHostToDevice) != hipSuccess)
    rc = SFS2D_E_HIP;
  if (rc) { plan_free(a); delete a; return rc == SFS2D_E_HIP ? set_err(ctx, rc, "attach: copy") : rc; }
  base->attached.push_back(a);
  *out = a;
  return 0;
}

static int bg_hist_impl(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int32_t chrom, int64_t* h2d,
                        int64_t* h1a, int64_t* h1b, int64_t* d_row);

int sfs2d_bg_hist(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int32_t chrom, int64_t* h2d,
                  int64_t* h1a, int64_t* h1b) {
  if (!ctx || !data || !prm || !h2d || !h1a || !h1b) return set_err(ctx, SFS2D_E_ARG, "null argument");
  return bg_hist_impl(ctx, data, prm, chrom, h2d, h1a, h1b, nullptr);
}

int sfs2d_bg_hist_dev(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int32_t chrom, int64_t* d_row) {
  if (!ctx || !data || !prm || !d_row) return set_err(ctx, SFS2D_E_ARG, "null argument");
  return bg_hist_impl(ctx, data, prm, chrom, nullptr, nullptr, nullptr, d_row);
}

// d_row: the histograms as one device row (k_bg_rows_get's layout) instead of host arrays
static int bg_hist_impl(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* prm, int32_t chrom, int64_t* h2d,
                        int64_t* h1a, int64_t* h1b, int64_t* d_row) {
  if (chrom < -1 || chrom >= data->nchrom) return set_err(ctx, SFS2D_E_ARG, "chrom out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  KParams K;
  int rc = make_kparams(ctx, prm, data->nchrom, &K);
  if (rc) return rc;
  // one pseudo-chromosome: all tiles accumulate into background 0
  sfs2d_plan pl;
  pl.ctx = ctx; pl.data = data; pl.prm = *prm; pl.K = K; pl.K.nchrom = 1;
  pl.do_bg = true; pl.do_seg = false;
  pl.bg_lds = ((size_t)K.nh + WAVE) * 4;
  pl.lds_hist = pl.bg_lds <= 150 * 1024;
  const int c0 = chrom < 0 ? 0 : chrom, c1 = chrom < 0 ? data->nchrom : chrom + 1;
  const int64_t T = 16384;
  for (int c = c0; c < c1; ++c)
    for (int64_t s = data->chrom_off[c]; s < data->chrom_off[c + 1];) {   // (edges on multiples of 4, as plans)
      const int64_t e = std::min<int64_t>((s & ~int64_t(3)) + T, data->chrom_off[c + 1]);
      Tile t{};
      t.chrom = 0; t.begin = (uint32_t)s; t.end = (uint32_t)e;
      t.cb = (uint32_t)data->chrom_off[c]; t.ce = (uint32_t)data->chrom_off[c + 1];
      pl.tiles.push_back(t);
      s = e;
    }
  // chrom_off for pseudo-chromosome 0 is only read by segmentation (disabled)
  std::vector<uint32_t> hist((size_t)REPL * K.nh, 0);
  rc = 0;
  rc = rc ? rc : dalloc(ctx, &pl.d_tiles, pl.tiles.size());
  rc = rc ? rc : dalloc(ctx, &pl.d_repl, (size_t)REPL * K.nh);
  rc = rc ? rc : dalloc(ctx, &pl.d_bcount, 1);
  rc = rc ? rc : dalloc(ctx, &pl.d_err, 1);
  hipError_t e = hipSuccess;
  if (!rc) {
    if (!pl.tiles.empty()) e = hipMemcpyAsync(pl.d_tiles, pl.tiles.data(), sizeof(Tile) * pl.tiles.size(), hipMemcpyHostToDevice, CTX_STREAM(ctx));
    if (e == hipSuccess) e = hipMemsetAsync(pl.d_repl, 0, sizeof(uint32_t) * REPL * K.nh, CTX_STREAM(ctx));
    if (e == hipSuccess) e = hipMemsetAsync(pl.d_err, 0, 4, CTX_STREAM(ctx));
    if (e == hipSuccess) e = hipMemsetAsync(pl.d_bcount, 0, 4, CTX_STREAM(ctx));
    if (e == hipSuccess && pl.lds_hist && pl.bg_lds > 64 * 1024) grant_lds<Prep>(ctx, pl.bg_lds);
    if (e == hipSuccess) rc = launch_prep(&pl, false);
    // (rc: a selection outside the table launched nothing; reported below, after the buffers are freed)
    if (!rc && e == hipSuccess && d_row) {
      const int W = K.h1b + K.n2 + 2;
      hipLaunchKernelGGL(k_bg_rows_get, dim3((unsigned)((W + 255) / 256), 1u), dim3(256), 0, CTX_STREAM(ctx), pl.K,
                         pl.d_repl, (unsigned long long)K.nh, pl.d_bcount, (long long*)d_row, (long long)W);
      e = hipGetLastError();
    } else if (!rc && e == hipSuccess) {
      e = hipMemcpyAsync(hist.data(), pl.d_repl, sizeof(uint32_t) * REPL * K.nh, hipMemcpyDeviceToHost, CTX_STREAM(ctx));
    }
    uint32_t err = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&err, pl.d_err, 4, hipMemcpyDeviceToHost, CTX_STREAM(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(CTX_STREAM(ctx));
    if (e == hipSuccess && err) rc = (err & ERR_KEY) ? set_err(ctx, SFS2D_E_KEY, "allele count above 2*pop_size")
                                                     : set_err(ctx, SFS2D_E_GRID, "folded 2D bin outside the grid");
  }
  hipFree(pl.d_tiles); hipFree(pl.d_repl); hipFree(pl.d_err); hipFree(pl.d_bcount);
  pl.d_tiles = nullptr; pl.d_repl = nullptr; pl.d_err = nullptr; pl.d_bcount = nullptr;
  if (e != hipSuccess) return set_err(ctx, SFS2D_E_HIP, std::string("bg_hist: ") + hipGetErrorString(e));
  if (rc || d_row) return rc;
  for (int k = 0; k < K.h1b + K.n2 + 1; ++k) {
    int64_t s = 0;
    for (int r = 0; r < REPL; ++r) s += hist[(size_t)r * K.nh + k];
    if (k < K.nb2) h2d[k] = s;
    else if (k < K.h1b) h1a[k - K.h1a] = s;
    else h1b[k - K.h1b] = s;
  }
  return 0;
}

int sfs2d_scan(sfs2d_ctx* ctx, const sfs2d_data* data, const sfs2d_params* params, const double* bg2d,
               const double* bg1a, const double* bg1b, sfs2d_window* out_host, int64_t cap, int64_t* nrec_out) {
  sfs2d_plan* pl = nullptr;
  int rc = sfs2d_plan_create(ctx, data, params, &pl);
  if (rc) return rc;
  if (params->bg_mode == SFS2D_BG_SUPPLIED) rc = sfs2d_plan_set_background(pl, bg2d, bg1a, bg1b);
  if (!rc) rc = sfs2d_plan_run(pl, nullptr);
  if (!rc) rc = sfs2d_plan_check(pl);
  if (!rc) rc = sfs2d_plan_read(pl, out_host, cap, nrec_out);
  else if (nrec_out) *nrec_out = pl->nrec;
  std::string keep = ctx->err;
  sfs2d_plan_destroy(pl);
  ctx->err = keep;
  return rc;
}

}  // extern "C"
