// sfs2d_proj.hpp -- projected window spectra (included by sfs2d.hip after sfs2d_spec.hpp).
//
// The joint SFS of chosen records of a plan's last run, projected down hypergeometrically to a common sample size
// (m1, m2) and summed into groups: what dadi's from_data_dict(projections=...) and easySFS
// do, from the packed (ref, alt) counts that are resident.  A member SNP (the scan's own membership, as k_div_win
// takes it) with called counts n_k = r_k + a_k >= m_k in both populations is used and adds
//   h(j1; n1, a1, m1) h(j2; n2, a2, m2),   h(j; n, a, m) = C(a, j) C(n - a, m - j) / C(n, m),
// to bin (j1, j2) of a dense (m1 + 1) x (m2 + 1) grid over its support max(0, m - (n - a)) <= j <= min(m, a); any
// other member is dropped.  A group's row is [grid, int64 fixed point 2^-e | n_used | n_dropped] --
// SFS2D_PROJ_ROW_WORDS; every term is rounded to nearest once and the sums are integer: the rows do not depend on
// the schedule.
#pragma once

#include <cmath>

#include "sfs2d_kernels.hpp"

namespace sfs2dk {

constexpr int PROJ_BLOCK = 256;   // k_proj_win workgroup: four wavefronts streaming one entry together
constexpr int PROJ_ROWS = 4;      // rows of 256 SNPs whose loads are in flight together (two loads each when !CNT)
constexpr int PROJ_LF = 511;      // ln k! for k = 0 .. 510: u8 counts, n = r + a <= 510
constexpr int PROJ_CHUNK = 1024;  // SNPs of one selection entry cut from a chromosome entry (one block of rows)

struct ProjSel {   // one selection entry: a record of the last run (its own range) or, rec == 0xffffffff, [begin, end)
  uint32_t rec, grp, begin, end;
};

// The weight h(j; n, a, m) from the table lf[k] = ln k!, in two steps so that a SNP's j-independent part is formed
// once: c = proj_lnc(lf, n, a, m), then proj_w(lf, c, n, a, m, j) for j in the support (outside it: exactly 0; a
// support of one bin -- m == n, a == 0 or a == n among them -- has weight exactly 1).  Host and device evaluate
// this source (sfs2d_project_weights).  Needs a <= n, m <= n, n < PROJ_LF.
__host__ __device__ inline double proj_lnc(const double* lf, uint32_t n, uint32_t a, uint32_t m) {
  return (lf[a] + lf[n - a]) - (lf[n] - lf[m] - lf[n - m]);
}
__host__ __device__ inline double proj_w(const double* lf, double c, uint32_t n, uint32_t a, uint32_t m, uint32_t j) {
  const uint32_t r = n - a, lo = m > r ? m - r : 0u, hi = m < a ? m : a;
  if (j < lo || j > hi) return 0.0;
  if (lo == hi) return 1.0;
  return exp(c - (lf[j] + lf[a - j]) - (lf[m - j] + lf[r - (m - j)]));
}

extern __shared__ __attribute__((aligned(16))) unsigned long long proj_lds[];

// The projection of the SNPs [b, e), by a whole workgroup of PROJ_BLOCK lanes (k_proj_win's entries, k_proj_scan's
// records): rows of 256 SNPs, PROJ_ROWS rows' loads in flight (every lane loads: past the range its last SNP
// again, dropped by a select -- no branch between the loads); counts alone on a counts plan (cls_word gives the
// membership), counts and the stored bins word otherwise.  Per row of SNPs the ballots' counts of used and dropped
// members go to count(nu, nd) on each wavefront's first lane.  A lane owns its SNP and walks the SNP's support
// rectangle [l1, h1] x [l2, h2] itself -- (d1 + 1)(d2 + 1) bins at most, d_k = n_k - m_k: one exp per bin of the
// rectangle and one per row of it, each term rounded to nearest at 2^-e (scale = 2^e) and, when not zero, handed
// to add(j1, j2, t).  lf: the table of ln k!, in LDS.
template <bool CNT, class Count, class Add>
__device__ __forceinline__ void proj_walk(const KParams& P, const uint32_t* __restrict__ counts,
                                          const uint32_t* __restrict__ bins, const double* lf, uint32_t b, uint32_t e,
                                          uint32_t m1, uint32_t m2, double scale, Count count, Add add) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t r0 = b; r0 < e; r0 += PROJ_ROWS * PROJ_BLOCK) {
    uint32_t c[PROJ_ROWS], w[PROJ_ROWS];
#pragma unroll
    for (int j = 0; j < PROJ_ROWS; ++j) {
      const uint32_t k = r0 + PROJ_BLOCK * j + tid, kc = min(k, e - 1u);
      const uint32_t cv = counts[kc];
      c[j] = k < e ? cv : 0u;   // (counts 0: an SNP in no spectrum)
      if (!CNT) {
        const uint32_t wv = bins[kc];
        w[j] = k < e ? wv : 0u;   // (a bins word with no bin)
      }
    }
#pragma unroll
    for (int j = 0; j < PROJ_ROWS; ++j) {
      const uint32_t wj = CNT ? cls_word(P, c[j]) : w[j];
      const bool member = (bin_k2(wj) != 0u) | ((wj & B_LAST) != 0u);
      const uint32_t cj = c[j];
      const uint32_t r1 = cj & 0xffu, a1 = (cj >> 8) & 0xffu, r2 = (cj >> 16) & 0xffu, a2 = cj >> 24;
      const uint32_t n1c = r1 + a1, n2c = r2 + a2;   // u8 counts: n <= 510 < PROJ_LF
      const bool used = member & (n1c >= m1) & (n2c >= m2);
      const uint32_t nu = (uint32_t)__popcll(__ballot(used)), nd = (uint32_t)__popcll(__ballot(member & !used));
      if ((tid & (WAVE - 1)) == 0) count(nu, nd);
      if (used) {
        const uint32_t l1 = m1 > r1 ? m1 - r1 : 0u, h1 = min(m1, a1);
        const uint32_t l2 = m2 > r2 ? m2 - r2 : 0u, h2 = min(m2, a2);
        const double c1 = proj_lnc(lf, n1c, a1, m1), c2 = proj_lnc(lf, n2c, a2, m2);
        for (uint32_t j1 = l1; j1 <= h1; ++j1) {
          const double v1 = proj_w(lf, c1, n1c, a1, m1, j1) * scale;
          for (uint32_t j2 = l2; j2 <= h2; ++j2) {
            const unsigned long long t = (unsigned long long)__double2ll_rn(v1 * proj_w(lf, c2, n2c, a2, m2, j2));
            if (t) add(j1, j2, t);
          }
        }
      }
    }
  }
}

// Workgroup b takes the contiguous run [b nsel / G, (b + 1) nsel / G) of the selection, as k_spec_win.  Per entry:
// the SNP range from the record itself (rec_range), or the entry's own (a whole chromosome), projected by
// proj_walk and added as u64.
//   LDSH: into a u64 histogram of the whole row in LDS (non-returning ds_add_u64), flushed when the group changes
//   or the run ends -- every non-zero word one 64-bit device-scope atomic add into the group's row, zeroed in the
//   same pass -- and before the SNPs held could carry a word past 2^63 (hold_max SNPs, each adds at most 2^e to
//   a word).
//   !LDSH (rows that fit no LDS): the same adds as 64-bit global atomics straight into the group's row.
// n_used / n_dropped: one add per wavefront and row of SNPs.
template <bool CNT, bool LDSH>
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_win(KParams P, const uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ bins,
                                                         const sfs2d_window* __restrict__ recs,
                                                         const ProjSel* __restrict__ sel,
                                                         const double* __restrict__ lft,
                                                         unsigned long long* __restrict__ out, uint32_t nsel,
                                                         uint32_t nrec, uint32_t ngroups, uint32_t nsnp, uint32_t m1,
                                                         uint32_t m2, double scale, unsigned long long hold_max) {
  __shared__ double lf[PROJ_LF + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t w2 = m2 + 1u, ngrid = (m1 + 1u) * w2, roww = ngrid + 2u;
  unsigned long long* H = proj_lds;
  for (uint32_t k = tid; k < PROJ_LF; k += PROJ_BLOCK) lf[k] = lft[k];
  if (LDSH)
    for (uint32_t k = tid; k < roww; k += PROJ_BLOCK) H[k] = 0ull;
  __syncthreads();
  uint32_t cur = 0xffffffffu;        // the group in the LDS histogram (none yet)
  unsigned long long held = 0;       // SNPs streamed into it since its last flush: bounds every word
  unsigned long long* row = out;
  auto flush = [&]() {
    __syncthreads();   // (every wavefront's LDS adds are in)
    for (uint32_t k = tid; k < roww; k += PROJ_BLOCK) {
      const unsigned long long v = H[k];
      if (v) {
        atomicAdd(row + k, v);
        H[k] = 0ull;
      }
    }
    __syncthreads();
  };
  const uint32_t lo = (uint32_t)((unsigned long long)blockIdx.x * nsel / gridDim.x);
  const uint32_t hi = (uint32_t)((unsigned long long)(blockIdx.x + 1u) * nsel / gridDim.x);
  for (uint32_t i = lo; i < hi; ++i) {
    // (the entry is the workgroup's: scalar values, uniform branches around the barriers)
    const uint32_t s = __builtin_amdgcn_readfirstlane(sel[i].rec), g = __builtin_amdgcn_readfirstlane(sel[i].grp);
    if (g >= ngroups) continue;   // (the library has checked it: never taken)
    uint32_t e, b;
    if (s == 0xffffffffu) {
      e = min(__builtin_amdgcn_readfirstlane(sel[i].end), nsnp);
      b = min(__builtin_amdgcn_readfirstlane(sel[i].begin), e);
    } else {
      if (s >= nrec) continue;   // (checked too)
      const RecRange rr = rec_range<true>(recs, s, nsnp);
      if (rr.flags) continue;   // no window of its own
      e = rr.e;
      b = rr.b;
    }
    if (b == e) continue;
    if (LDSH && cur != 0xffffffffu && (g != cur || held + (e - b) > hold_max)) {
      flush();
      held = 0;
    }
    cur = g;
    held += e - b;
    row = out + (size_t)g * roww;
    // (two address spaces: the adds stay LDS / global instructions, no flat pointer)
    auto add = [&](uint32_t k, unsigned long long v) {
      if (LDSH) atomicAdd(H + k, v);
      else atomicAdd(row + k, v);
    };
    proj_walk<CNT>(
        P, counts, bins, lf, b, e, m1, m2, scale,
        [&](uint32_t nu, uint32_t nd) {
          if (nu) add(ngrid, (unsigned long long)nu);
          if (nd) add(ngrid + 1u, (unsigned long long)nd);
        },
        [&](uint32_t j1, uint32_t j2, unsigned long long t) { add(j1 * w2 + j2, t); });
  }
  if (LDSH && cur != 0xffffffffu) flush();
}

}  // namespace sfs2dk
