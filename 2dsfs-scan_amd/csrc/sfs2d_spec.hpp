// sfs2d_spec.hpp -- window spectra (included by sfs2d.hip after sfs2d_kernels.hpp).
//
// The spectra themselves of chosen records of a plan's last run, summed into groups: what
// the scan reduces to T2D / T1D and four totals per window, returned as the x_k.  A selection is a list of
// (record, group) pairs; group g's row is the sum over its entries of the record's
//   [ 2D grid, nb2 = (n1+1)(n2+1) bins, row-major (x1, x2): the flat key k2 of the scan; (0,0) stays 0, the last
//     bin (n1, n2) holds the B_LAST SNPs
//   | pop-1 folded 1D spectrum, n1p+1 entries: the inner bins 1 .. n1p-1 (entries 0 and n1p stay 0)
//   | pop-2 folded 1D spectrum, n2p+1 entries ]
// as int64 -- SFS2D_SPEC_ROW_WORDS.  Integer sums: the rows do not depend on the schedule.
#pragma once

#include "sfs2d_kernels.hpp"

namespace sfs2dk {

constexpr int SPEC_BLOCK = 256;   // k_spec_win workgroup: four wavefronts streaming one record together
constexpr int SPEC_ROWS = 8;      // rows of 256 SNPs whose loads are in flight together

struct SpecSel {   // one selection entry: record index of the last run, group
  uint32_t rec, grp;
};

extern __shared__ __attribute__((aligned(16))) uint32_t spec_lds[];

// Workgroup b takes the contiguous run [b nsel / G, (b + 1) nsel / G) of the selection.  Per entry: the SNP range
// [begin, end) from the record itself (as k_div_win: not from the slot table), all 256 lanes over rows of 256
// SNPs, SPEC_ROWS rows' loads in flight (every lane loads: past the range its last SNP again, dropped by a select
// -- no branch between the loads), membership and bins as the scan takes them (cls_word of the counts on a counts
// plan, the stored bins word otherwise): one 2D add and up to two 1D adds per member SNP.
//   LDSH: into a u32 histogram of the whole row in LDS (non-returning ds_add_u32), flushed when the group changes
//   or the run ends -- every non-zero word one 64-bit device-scope atomic add into the group's row, zeroed in the
//   same pass -- so consecutive entries of one group cost one flush per workgroup; and before a record that could
//   carry a u32 word past 2^32 - 1.
//   !LDSH (rows that fit no LDS): the same adds as 64-bit global atomics straight into the group's row.
template <bool CNT, bool LDSH>
__global__ __launch_bounds__(SPEC_BLOCK) void k_spec_win(KParams P, const uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ bins,
                                                         const sfs2d_window* __restrict__ recs,
                                                         const SpecSel* __restrict__ sel,
                                                         unsigned long long* __restrict__ out, uint32_t nsel,
                                                         uint32_t nrec, uint32_t ngroups, uint32_t nsnp) {
  const uint32_t tid = threadIdx.x;
  const uint32_t nb2 = (uint32_t)P.nb2, o1 = nb2, o2 = nb2 + (uint32_t)P.n1p + 1u, roww = o2 + (uint32_t)P.n2p + 1u;
  const uint32_t* __restrict__ src = CNT ? counts : bins;   // 4 B/SNP either way
  uint32_t* H = spec_lds;
  if (LDSH) {
    for (uint32_t k = tid; k < roww; k += SPEC_BLOCK) H[k] = 0u;
    __syncthreads();
  }
  const uint32_t lo = (uint32_t)((unsigned long long)blockIdx.x * nsel / gridDim.x);
  const uint32_t hi = (uint32_t)((unsigned long long)(blockIdx.x + 1u) * nsel / gridDim.x);
  uint32_t cur = 0xffffffffu;        // the group in the LDS histogram (none yet)
  unsigned long long held = 0;       // SNPs streamed into it since its last flush: bounds every u32 word
  unsigned long long* row = out;
  auto flush = [&]() {
    __syncthreads();   // (every wavefront's LDS adds are in)
    for (uint32_t k = tid; k < roww; k += SPEC_BLOCK) {
      const uint32_t v = H[k];
      if (v) {
        atomicAdd(row + k, (unsigned long long)v);
        H[k] = 0u;
      }
    }
    __syncthreads();
  };
  for (uint32_t i = lo; i < hi; ++i) {
    // (the entry is the workgroup's: scalar values, uniform branches around the barriers)
    const uint32_t s = __builtin_amdgcn_readfirstlane(sel[i].rec), g = __builtin_amdgcn_readfirstlane(sel[i].grp);
    if (s >= nrec || g >= ngroups) continue;   // (the library has checked both: never taken)
    if (__builtin_amdgcn_readfirstlane(recs[s].flags) & (SFS2D_W_EMPTY | SFS2D_W_EXTRA)) continue;   // no window of its own
    const uint32_t e = min(__builtin_amdgcn_readfirstlane(recs[s].end), nsnp);   // (never past the data set)
    const uint32_t b = min(__builtin_amdgcn_readfirstlane(recs[s].begin), e);
    if (b == e) continue;
    if (LDSH && cur != 0xffffffffu && (g != cur || held + (e - b) > 0xffffffffull)) {
      flush();
      held = 0;
    }
    cur = g;
    held += e - b;
    row = out + (size_t)g * roww;
    for (uint32_t r0 = b; r0 < e; r0 += SPEC_ROWS * SPEC_BLOCK) {
      uint32_t w[SPEC_ROWS];
#pragma unroll
      for (int j = 0; j < SPEC_ROWS; ++j) {
        const uint32_t k = r0 + SPEC_BLOCK * j + tid, kc = min(k, e - 1u);
        const uint32_t v = src[kc];
        w[j] = k < e ? v : 0u;   // (0: counts of an SNP in no spectrum / a bins word with no bin)
      }
#pragma unroll
      for (int j = 0; j < SPEC_ROWS; ++j) {
        const uint32_t wj = CNT ? cls_word(P, w[j]) : w[j];
        const uint32_t k2 = (wj & B_LAST) ? nb2 - 1u : bin_k2(wj), g1 = bin_g1(wj), g2 = bin_g2(wj);
        if (LDSH) {
          if (k2) atomicAdd(&H[k2], 1u);
          if (g1) atomicAdd(&H[o1 + g1], 1u);
          if (g2) atomicAdd(&H[o2 + g2], 1u);
        } else {
          if (k2) atomicAdd(row + k2, 1ull);
          if (g1) atomicAdd(row + o1 + g1, 1ull);
          if (g2) atomicAdd(row + o2 + g2, 1ull);
        }
      }
    }
  }
  if (LDSH && cur != 0xffffffffu) flush();
}

}  // namespace sfs2dk
