"""Similarity of sets of fingerprints on the device (csrc/fp_sim.hip; DESIGN.md 2.9 "Fingerprints and similarity").

A set is an int64 tensor [n, FP_WORDS] of 64-bit patterns, as `molecule.fingerprints` writes them (`Fingerprints.fp[f]`) or `stack`
builds from assembled molecules.  `tanimoto` is the all-pairs matrix, `nearest` the nearest neighbour of every row with the row sums
(no matrix in memory), `internal_diversity` one minus the mean similarity of the distinct pairs, `maxmin_pick` a MaxMin diverse subset.
For rows x, y: c = popcount(x & y), u = popcount(x) + popcount(y) - c, similarity = fp32(c) / fp32(u) rounded to nearest, and 1 for two
empty rows.  Every similarity and every index is exact; ties go to the lowest index.  The fingerprint is not RDKit's ECFP
(`molecule.fingerprints`), so the values are not RDKit's."""
from dataclasses import dataclass

import numpy as np
import torch

from . import hip
from .molecule import FP_WORDS

TILE_A = 256                     # rows a workgroup holds in registers, one per lane (PG_FP_TILE_A)
TILE_B = 64                      # rows of one LDS tile of the other set (PG_FP_TILE_B); a split of that set is a whole number of tiles


@dataclass
class Nearest:
    """Device tensors of one `nearest` call over the n rows of a."""
    sim: torch.Tensor            # fp32  [n] the largest similarity to a row of b; -1 without a candidate
    index: torch.Tensor          # int32 [n] the lowest row of b that attains it; -1 without a candidate
    sum: torch.Tensor            # fp64  [n] the sum of the row's fp32 similarities


@dataclass
class MaxMin:
    """Device tensors of one `maxmin_pick` call."""
    index: torch.Tensor          # int32 [k] the picked rows in pick order
    sim: torch.Tensor            # fp32  [k] the pick's largest similarity to the rows picked before it; -1 for the first


def _check_set(fn, t, what):
    if not torch.is_tensor(t) or t.dim() != 2 or t.size(1) != FP_WORDS or t.dtype != torch.int64:
        raise ValueError(f'phoregen_amd.similarity.{fn}: {what} must be an int64 tensor [n, {FP_WORDS}], not '
                         f'{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}'
                         f'{" of " + str(t.dtype) if torch.is_tensor(t) else ""}')
    if t.device.type != 'cuda':
        raise RuntimeError(f'phoregen_amd.similarity.{fn}: the similarity is a HIP kernel and {what} lives on {t.device}; there is no '
                           'CPU fallback')
    if not t.is_contiguous():
        raise ValueError(f'phoregen_amd.similarity.{fn}: {what} must be contiguous')
    if t.size(0) > 0x7fffffff:
        raise ValueError(f'phoregen_amd.similarity.{fn}: {what} has {t.size(0)} rows, at most 2**31 - 1')


def _pair(fn, a, b):
    _check_set(fn, a, 'a')
    if b is not None:
        _check_set(fn, b, 'b')
        if b.device != a.device:
            raise ValueError(f'phoregen_amd.similarity.{fn}: a lives on {a.device}, b on {b.device}')


def stack(mols, device):
    """The fingerprints of assembled molecules (`assemble(fingerprints=)`) as one set on `device`: int64 [n, FP_WORDS]."""
    rows = np.zeros((len(mols), FP_WORDS), dtype=np.uint64)
    for i, m in enumerate(mols):
        if 'fingerprint' not in m:
            raise ValueError(f'phoregen_amd.similarity.stack: molecule {i} carries no fingerprint (assemble(fingerprints=))')
        rows[i] = np.asarray(m['fingerprint'], dtype=np.uint64).reshape(FP_WORDS)
    return torch.from_numpy(rows.view(np.int64)).to(device)


@torch.no_grad()
def tanimoto(a, b=None):
    """The similarity of every row of a to every row of b (b=None: of a): fp32 [na, nb] on the device (pg_fp_tanimoto).  na * nb is
    at most 2**31 - 1; `nearest` needs no matrix."""
    _pair('tanimoto', a, b)
    b = a if b is None else b
    na, nb = a.size(0), b.size(0)
    if na * nb > 0x7fffffff:
        raise ValueError(f'phoregen_amd.similarity.tanimoto: {na} x {nb} elements exceed 2**31 - 1; use nearest(), or cut the sets')
    with torch.cuda.device(a.device):
        lib = hip.lib()
        out = torch.empty(na, nb, dtype=torch.float32, device=a.device)
        hip.check(lib.pg_fp_tanimoto(a.data_ptr(), na, b.data_ptr(), nb, out.data_ptr(), hip.stream_ptr()), 'pg_fp_tanimoto')
    return out


@torch.no_grad()
def nearest(a, b=None):
    """For every row of a its nearest neighbour among the rows of b (pg_fp_nearest): the largest similarity, the lowest row that
    attains it, and the fp64 sum of the row's similarities.  b=None: among the other rows of a (row i itself is left out).  A row
    without a candidate has similarity -1, index -1, sum 0."""
    _pair('nearest', a, b)
    same = b is None
    b = a if same else b
    na, nb = a.size(0), b.size(0)
    with torch.cuda.device(a.device):
        lib = hip.lib()
        out = Nearest(sim=torch.empty(na, dtype=torch.float32, device=a.device), index=torch.empty(na, dtype=torch.int32, device=a.device),
                      sum=torch.empty(na, dtype=torch.float64, device=a.device))
        hip.check(lib.pg_fp_nearest(a.data_ptr(), na, b.data_ptr(), nb, int(same), out.sim.data_ptr(), out.index.data_ptr(),
                                    out.sum.data_ptr(), hip.stream_ptr()), 'pg_fp_nearest')
    return out


def _diversity(total, n):
    """1 - total / (n (n - 1)) with `total` the sum of the similarities of all ordered pairs i != j; nan below two rows."""
    return float('nan') if n < 2 else 1.0 - float(total) / (n * (n - 1))


@torch.no_grad()
def internal_diversity(a):
    """One minus the mean similarity of the distinct pairs of a: 1 - sum_i nearest(a).sum[i] / (n (n - 1)); nan for n < 2.  One host
    read."""
    _check_set('internal_diversity', a, 'a')
    n = a.size(0)
    return _diversity(nearest(a).sum.sum().item() if n >= 2 else 0.0, n)


@torch.no_grad()
def maxmin_pick(a, k, first=0):
    """MaxMin diverse subset of k rows of a, starting from row `first` (pg_fp_maxmin): every further pick is the row whose largest
    similarity to the rows picked so far is smallest, the lowest index among equals.  No host read between the picks."""
    _check_set('maxmin_pick', a, 'a')
    n = a.size(0)
    for name, v in (('k', k), ('first', first)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'phoregen_amd.similarity.maxmin_pick: {name} must be an integer, not {v!r}')
    k, first = int(k), int(first)
    if not 0 <= k <= n or (n > 0 and not 0 <= first < n):
        raise ValueError(f'phoregen_amd.similarity.maxmin_pick: {k} picks from {n} rows, first {first} (0 <= k <= n, 0 <= first < n)')
    with torch.cuda.device(a.device):
        lib = hip.lib()
        out = MaxMin(index=torch.empty(k, dtype=torch.int32, device=a.device), sim=torch.empty(k, dtype=torch.float32, device=a.device))
        work = torch.empty(n, dtype=torch.float32, device=a.device)
        slots = torch.empty(k, dtype=torch.int64, device=a.device)
        hip.check(lib.pg_fp_maxmin(a.data_ptr(), n, k, first, out.index.data_ptr(), out.sim.data_ptr(), work.data_ptr(), slots.data_ptr(),
                                   hip.stream_ptr()), 'pg_fp_maxmin')
    return out
