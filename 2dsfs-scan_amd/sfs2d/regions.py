"""Region windows: a caller's list of intervals (genes, an inversion, candidate regions) scanned as windows.

A region is ``(chrom, first, last)``: ``first <= last`` are 1-based inclusive positions below 2**32 on one
chromosome of the data set; it holds the SNPs of that chromosome with ``first <= pos <= last`` (repeated positions
at a boundary are all inside; a SNP at position 0 is inside only when ``first == 0``).  Regions may overlap, nest,
repeat and come in any order; include/sfs2d.h (sfs2d_plan_create_regions) and DESIGN.md section 16 have the rest.

This module holds the host side: the ``Regions`` value the engine, the post-pass and the class methods pass around
(the list sorted stably by chromosome, as the library wants it, with the permutation back to the caller's order),
the BED reader, and the numpy definition of a region's SNP range (``region_ranges``) the tests compare the device's
slot table against.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

__all__ = ["Regions", "read_bed", "region_ranges"]

_POS_MAX = (1 << 32) - 1


class Regions:
    """A list of regions against one data set's chromosome names.

    ``chrom`` (int32), ``first`` / ``last`` (uint32): the regions in SLOT order -- sorted stably by chromosome
    index, so a chromosome's regions keep the caller's order among themselves.  ``order[s]`` is the caller's index
    of slot s, ``slot[i]`` the slot of the caller's region i.  ``names[i]`` (caller's order) is the region's name
    or None; ``keys()[i]`` its row key: the name, or ``"<chrom> <first>-<last>"``.  Two regions with one key are a
    ValueError (name the repeats)."""

    def __init__(self, chrom_names: Sequence[str], items):
        chrom_names = list(chrom_names)
        index = {c: i for i, c in enumerate(chrom_names)}
        cs, fs, ls, names = [], [], [], []
        for k, it in enumerate(items):
            if len(it) not in (3, 4):
                raise ValueError(f"region {k}: expected (chrom, first, last[, name]), got {it!r}")
            c, f, l = it[0], int(it[1]), int(it[2])
            if c not in index:
                raise ValueError(f"region {k}: chromosome {c!r} is not in the data")
            if not 0 <= f <= l <= _POS_MAX:
                raise ValueError(f"region {k}: need 0 <= first <= last < 2**32, got {f}-{l}")
            cs.append(index[c]); fs.append(f); ls.append(l)
            names.append(None if len(it) == 3 or it[3] is None else str(it[3]))
        if not cs:
            raise ValueError("an empty region list")
        c = np.asarray(cs, np.int32)
        self.chrom_names = chrom_names
        self.order = np.argsort(c, kind="stable").astype(np.int64)
        self.slot = np.empty(len(c), np.int64)
        self.slot[self.order] = np.arange(len(c), dtype=np.int64)
        self.chrom = np.ascontiguousarray(c[self.order])
        self.first = np.ascontiguousarray(np.asarray(fs, np.uint32)[self.order])
        self.last = np.ascontiguousarray(np.asarray(ls, np.uint32)[self.order])
        self.names: List[Optional[str]] = names
        self._keys = [n if n is not None else f"{chrom_names[ci]} {f}-{l}" for n, ci, f, l in zip(names, cs, fs, ls)]
        seen = set()
        for k in self._keys:
            if k in seen:
                raise ValueError(f"duplicate region key {k!r} (give repeated regions distinct names)")
            seen.add(k)

    @classmethod
    def from_bed(cls, packed, path) -> "Regions":
        """The regions of BED file ``path`` against ``packed``'s chromosome names."""
        return cls(packed.chrom_names, read_bed(path))

    @classmethod
    def of(cls, packed, regions) -> "Regions":
        """``regions`` as a Regions against ``packed``: a Regions (its chromosome names must be the data's), a BED
        path, or an iterable of ``(chrom_name, first, last[, name])`` tuples."""
        if isinstance(regions, cls):
            if list(regions.chrom_names) != list(packed.chrom_names):
                raise ValueError("the Regions were built against another data set's chromosome names")
            return regions
        if isinstance(regions, (str, bytes)) or hasattr(regions, "__fspath__"):
            return cls.from_bed(packed, regions)
        return cls(packed.chrom_names, regions)

    def __len__(self) -> int:
        return len(self.chrom)

    def keys(self) -> List[str]:
        """Row keys in the caller's order."""
        return list(self._keys)

    def slot_keys(self) -> List[str]:
        """Row keys in slot order (record i of a regions plan is ``slot_keys()[i]``)."""
        return [self._keys[int(i)] for i in self.order]

    def lengths(self) -> np.ndarray:
        """``last - first + 1`` per slot (int64): the per-site divisor of a region."""
        return self.last.astype(np.int64) - self.first.astype(np.int64) + 1


def read_bed(path) -> list:
    """``(chrom_name, first, last[, name])`` tuples of a BED file.  BED is 0-based half-open, so
    ``first = start + 1``, ``last = end``; ``start >= end`` (an interval without a site) is a ValueError naming the
    line.  Blank lines and ``#`` / ``track`` / ``browser`` lines are skipped; column 4, when present, is the name."""
    out = []
    with open(path, "r") as fh:
        for ln, line in enumerate(fh, start=1):
            s = line.strip()
            if not s or s.startswith("#") or s.split(None, 1)[0] in ("track", "browser"):
                continue
            f = s.split("\t") if "\t" in s else s.split()
            try:
                if len(f) < 3:
                    raise ValueError("fewer than 3 columns")
                start, end = int(f[1]), int(f[2])
            except ValueError as e:
                raise ValueError(f"{path}: line {ln}: {e}") from None
            if start < 0 or start >= end:
                raise ValueError(f"{path}: line {ln}: need 0 <= start < end, got {start} {end}")
            out.append((f[0], start + 1, end) + ((f[3],) if len(f) > 3 and f[3] not in ("", ".") else ()))
    return out


def region_ranges(packed, regions: Regions):
    """(begin, end), int64 per slot: region s holds SNPs [begin[s], end[s]) of ``packed`` -- begin the chromosome's
    first SNP with pos >= first, end its first SNP with pos >= last + 1 (begin == end: an empty region)."""
    off = np.asarray(packed.chrom_off, np.int64)
    pos = np.asarray(packed.pos).astype(np.int64)
    begin = np.zeros(len(regions), np.int64)
    end = np.zeros(len(regions), np.int64)
    for s, (c, f, l) in enumerate(zip(regions.chrom.tolist(), regions.first.tolist(), regions.last.tolist())):
        lo, hi = int(off[c]), int(off[c + 1])
        begin[s] = lo + np.searchsorted(pos[lo:hi], f, side="left")
        end[s] = lo + np.searchsorted(pos[lo:hi], l + 1, side="left")
    return begin, end
