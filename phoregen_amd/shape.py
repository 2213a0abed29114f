"""3D shape and feature ("colour") similarity of molecules on the device (csrc/shape_sim.hip; DESIGN.md 2.9 "Shape").

Every molecule sampled for one pharmacophore lies in that pharmacophore's frame (`molecule.geometry_for` relies on the same), so two
molecules are compared where they lie: Gaussian-volume overlap with no alignment search.  A kept atom of element e is the Gaussian
P exp(-alpha_e |r - x|^2) with P = 2 sqrt(2) and alpha_e = KAPPA / R_e^2 (R_e from VDW_RADIUS_PM; one atom then integrates to
4/3 pi R_e^3).  For molecules A, B

    V(A, B) = sum_ij P^2 (pi / (a_i + a_j))^(3/2) exp(-(a_i a_j / (a_i + a_j)) d_ij^2)            first order only, no hydrogens
    C(A, B) = sum_ij popcount(fp_i & fp_j) P^2 (pi / (2 a_c))^(3/2) exp(-(a_c / 2) d_ij^2)       fp = `Features.atom_fp`, a_c = KAPPA / r_c^2
    ST = V(A, B) / (V(A, A) + V(B, B) - V(A, B)),  CT the same over C;  0 where the denominator is not positive
    score = (1 - w) ST + w CT

in fp32.  An empty molecule is similar to nothing, itself included.  A set built without features has no colour: its colour overlaps
and similarities are 0.  A pair's values are bit-identical wherever the two molecules sit in their sets, however the other set is
tiled or split, from `similarity` and from `nearest`, and whether the set was packed from a sampler result or from assembled
molecules; V(A, B) and V(B, A) may differ in the last bits.

`shape_set` packs a sampler result, `from_molecules` assembled molecules (the counterpart of `similarity.stack`), `from_mol_block` a
V2000 block such as the reference ligand; `concat` joins sets.  `similarity` is the all-pairs matrix, `nearest` the nearest neighbour
of every row with the row sums (no matrix in memory), `internal_diversity` one minus the mean score of the distinct pairs.

The radii are Bondi's and Mantina's values written from memory, and the colour radius is a design choice, not a calibration: the
values are not ROCS's or RDKit's.  Molecules that do not share a frame -- two runs against different pharmacophores, a reference
ligand in its crystal frame -- are overlaid first: `align` searches the best rigid pose of one molecule on the other (csrc/shape_align.hip;
DESIGN.md 2.9 "Shape alignment"), `frames` gives the principal frames it starts from, `transformed` applies a result.  Out of scope:
higher-order volume corrections, hydrogens, colour for a mol-block reference, MaxMin picks by shape, a shape filter inside
`sample_valid`."""
import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import hip
from . import molecule as M
from .similarity import Nearest, _diversity
from .utils.sample_utils import ATOM_TYPES

# van der Waals radii in pm, in ATOM_TYPES' order (B C N O F Si P S Cl Br I): Bondi's values, Mantina's for B -- written from memory,
# not checked against a table.  The table's only copy: the kernel and the tests' restatement are both handed it.
VDW_RADIUS_PM = (192, 170, 155, 152, 147, 210, 180, 180, 175, 185, 198)
P = 2.0 * math.sqrt(2.0)
KAPPA = math.pi / (4.0 * math.pi / (3.0 * P)) ** (2.0 / 3.0)        # about 2.41798793: one atom integrates to 4/3 pi R^3
TILE_A = 16                      # rows of a that a workgroup owns, a wave taking one pair of molecules at a time (PG_SHAPE_TILE_A)
TILE_B = 16                      # molecules of one LDS tile of b (PG_SHAPE_TILE_B); a split of b is a whole number of tiles
SHAPE_EMPTY = 1                  # no kept atom
SHAPE_NONFINITE = 2              # a kept atom with a non-finite coordinate
SHAPE_UNSELECTED = 4             # left out by `select`
SHAPE_NAMES = {SHAPE_EMPTY: 'EMPTY', SHAPE_NONFINITE: 'NONFINITE', SHAPE_UNSELECTED: 'UNSELECTED'}
_SYMBOL_Z = {s: z for z, s in M.ELEMENT_SYMBOL.items()}


@dataclass(frozen=True)
class ShapeOptions:
    radii_pm: tuple = VDW_RADIUS_PM          # per class of ATOM_TYPES
    colour_radius_pm: float = 100            # r_c of the colour Gaussians: a design choice, not calibrated

    def alphas(self):
        """alpha of every class, then the colour alpha, in 1 / Angstrom^2, as Python floats (inf for a zero radius: the library
        refuses it)."""
        radii = tuple(self.radii_pm) + (self.colour_radius_pm,)
        if len(radii) != len(ATOM_TYPES) + 1:
            raise ValueError(f'phoregen_amd.shape.ShapeOptions: radii_pm must hold {len(ATOM_TYPES)} radii, not {len(radii) - 1}')
        return [KAPPA / (float(r) / 100.0) ** 2 if float(r) != 0.0 else math.inf for r in radii]


def _alpha_arg(options):
    return (C.c_float * hip.PG_SHAPE_N_ALPHA)(*options.alphas())


@dataclass
class ShapeSet:
    """Device tensors of one packed set of n molecules."""
    atoms: torch.Tensor          # fp32  [A, 4] x, y, z, and as bits class | feature byte << 8 (-1: a dropped atom)
    mol: torch.Tensor            # int32 [n, 2] first atom row, atoms; an empty row has no atoms
    status: torch.Tensor         # int32 [n]    SHAPE_* bits; a row with any bit is an empty row
    self_shape: torch.Tensor     # fp32  [n]    V(A, A) in Angstrom^3
    self_colour: torch.Tensor    # fp32  [n]    C(A, A); 0 without colour
    has_colour: bool
    options: ShapeOptions = field(default_factory=ShapeOptions)

    @property
    def n(self):
        return self.mol.size(0)


def _need_cuda(fn, dev):
    if torch.device(dev).type != 'cuda':
        raise RuntimeError(f'phoregen_amd.shape.{fn}: the shape overlap is a HIP kernel and the set lives on {dev}; there is no CPU fallback')


def _check_options(fn, options):
    if not isinstance(options, ShapeOptions):
        raise ValueError(f'phoregen_amd.shape.{fn}: options must be a ShapeOptions, not {options!r}')


def _launch_pack(lib, cls, lig_off, pos, pos_fs, atom_fp, select, B, F, n_lig, max_n, alpha, atoms, mol, status):
    """pg_shape_pack on the current stream.  A graph above MAX_ATOMS or a bad alpha is the library's error: nothing is launched and
    the outputs are not written."""
    M._check_arrays('shape_set', cls.device, [(cls, torch.int8), (lig_off, torch.int32), (atoms, torch.float32), (mol, torch.int32),
                                             (status, torch.int32)] + ([(atom_fp, torch.uint8)] if atom_fp is not None else [])
                    + ([(select, torch.uint8)] if select is not None else []))
    if (lig_off.numel() != B + 1 or cls.numel() != F * n_lig or atoms.numel() != 4 * F * n_lig or mol.numel() != 2 * F * B
            or status.numel() != F * B or (atom_fp is not None and atom_fp.numel() != F * n_lig)
            or (select is not None and select.numel() != F * B)):
        raise ValueError(f'phoregen_amd.shape.shape_set: sizes of the offsets, arrays and outputs do not fit {F} frames x {B} graphs, '
                         f'{n_lig} atom rows')
    hip.check(lib.pg_shape_pack(cls.data_ptr(), lig_off.data_ptr(), pos.data_ptr(), pos_fs, hip.ptr(atom_fp), hip.ptr(select), B, F, n_lig,
                                max_n, alpha, atoms.data_ptr(), mol.data_ptr(), status.data_ptr(), hip.stream_ptr()), 'pg_shape_pack')


def _launch_self(lib, atoms, mol, alpha, self_shape, self_colour):
    """pg_shape_self on the current stream; self_colour may be None."""
    hip.check(lib.pg_shape_self(atoms.data_ptr(), atoms.size(0), mol.data_ptr(), mol.size(0), alpha, self_shape.data_ptr(),
                                hip.ptr(self_colour), hip.stream_ptr()), 'pg_shape_self')


def _set_args(s):
    return (s.atoms.data_ptr(), s.atoms.size(0), s.mol.data_ptr(), s.self_shape.data_ptr(), s.self_colour.data_ptr(), s.n)


def _launch_similarity(lib, a, b, alpha, shape_out, colour_out):
    """pg_shape_similarity on the current stream; colour_out may be None."""
    hip.check(lib.pg_shape_similarity(*_set_args(a), *_set_args(b), alpha, shape_out.data_ptr(), hip.ptr(colour_out), hip.stream_ptr()),
              'pg_shape_similarity')


def _launch_nearest(lib, a, b, same, has_colour, w, alpha, out):
    """pg_shape_nearest on the current stream.  A weight outside [0, 1] is the library's error: nothing is launched."""
    hip.check(lib.pg_shape_nearest(*_set_args(a), *_set_args(b), int(same), int(has_colour), w, alpha, out.sim.data_ptr(),
                                   out.index.data_ptr(), out.sum.data_ptr(), hip.stream_ptr()), 'pg_shape_nearest')


def _pack(fn, cls, lig_off, pos, pos_fs, atom_fp, select, B, F, n_lig, max_n, options):
    dev = cls.device
    with torch.cuda.device(dev):
        lib = hip.lib()
        alpha = _alpha_arg(options)
        atoms = torch.empty(F * n_lig, 4, dtype=torch.float32, device=dev)
        mol = torch.empty(F * B, 2, dtype=torch.int32, device=dev)
        status = torch.empty(F * B, dtype=torch.int32, device=dev)
        self_shape = torch.zeros(F * B, dtype=torch.float32, device=dev)
        self_colour = torch.zeros(F * B, dtype=torch.float32, device=dev)
        _launch_pack(lib, cls, lig_off, pos, pos_fs, atom_fp, select, B, F, n_lig, max_n, alpha, atoms, mol, status)
        _launch_self(lib, atoms, mol, alpha, self_shape, self_colour if atom_fp is not None else None)
    return ShapeSet(atoms=atoms, mol=mol, status=status, self_shape=self_shape, self_colour=self_colour, has_colour=atom_fp is not None,
                    options=options)


@torch.no_grad()
def shape_set(results, frames='final', screen=None, features=None, select=None, options=ShapeOptions()):
    """The molecules of a `sample` / `sample_batch` result as one set of F * B rows in (frame, graph) order (pg_shape_pack, then
    pg_shape_self), no host read beyond the screen's.  screen: a `Screen` of this result and frames (default: a new one).  features: a
    `Features` computed from that screen; it gives the set its colour (`atom_fp`).  select: bool [F, B], the rows to keep (default:
    `screen.valid`); every other row is an empty row with SHAPE_UNSELECTED.  A row without a kept atom (SHAPE_EMPTY) or with a
    non-finite coordinate on a kept atom (SHAPE_NONFINITE) is an empty row too."""
    _check_options('shape_set', options)
    _, pos, _, F, (_, _, pos_fs) = M._frames(results, frames)
    dev = pos.device
    _need_cuda('shape_set', dev)
    if features is not None and not isinstance(features, M.Features):
        raise ValueError(f'phoregen_amd.shape.shape_set: features= must be a Features, not {type(features).__name__}')
    sc = M._resolve('shape_set', results, frames, screen, where='phoregen_amd.shape', features=features)
    M._check_rows('shape_set', pos, F, 3, 'coordinates', dev)
    B, N = len(sc.num_atoms), pos.size(-2)
    if select is None:
        select = sc.valid
    if not torch.is_tensor(select) or select.dtype != torch.bool or tuple(select.shape) != (F, B) or select.device != dev:
        raise ValueError(f'phoregen_amd.shape.shape_set: select must be a bool tensor [{F}, {B}] on {dev}, not '
                         f'{tuple(select.shape) if torch.is_tensor(select) else type(select).__name__}')
    atom_fp = None
    if features is not None:
        atom_fp = features.atom_fp
        if tuple(atom_fp.shape) != (F, N) or atom_fp.dtype != torch.uint8 or atom_fp.device != dev:
            raise ValueError(f'phoregen_amd.shape.shape_set: features.atom_fp must be uint8 [{F}, {N}] on {dev}')
    return _pack('shape_set', sc.cls, sc.lig_off, pos, pos_fs, atom_fp, select.to(torch.uint8).contiguous(), B, F, N,
                 max(sc.num_atoms, default=0), options)


def _from_arrays(fn, elements, positions, fps, device, options):
    """One set from per-molecule lists of atomic numbers, [n, 3] coordinates and (or None) feature bytes: the same pack launch."""
    _check_options(fn, options)
    _need_cuda(fn, device)
    sizes = [len(e) for e in elements]
    N = sum(sizes)
    cls = np.full(N, -1, dtype=np.int8)
    pos = np.zeros((N, 3), dtype=np.float32)
    fp = np.zeros(N, dtype=np.uint8)
    n0 = 0
    for i, (el, xyz) in enumerate(zip(elements, positions)):
        n = len(el)
        xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
        if xyz.shape[0] != n:
            raise ValueError(f'phoregen_amd.shape.{fn}: molecule {i} has {n} elements and {xyz.shape[0]} positions')
        if n > M.MAX_ATOMS:
            raise ValueError(f'phoregen_amd.shape.{fn}: molecule {i} has {n} atoms, at most {M.MAX_ATOMS}')
        for k, z in enumerate(el):
            if int(z) not in ATOM_TYPES:
                raise ValueError(f'phoregen_amd.shape.{fn}: molecule {i} has an atom of atomic number {int(z)}, which is none of {ATOM_TYPES}')
            cls[n0 + k] = ATOM_TYPES.index(int(z))
        pos[n0:n0 + n] = xyz
        if fps is not None:
            row = np.asarray(fps[i], dtype=np.uint8).reshape(-1)
            if row.size != n:
                raise ValueError(f'phoregen_amd.shape.{fn}: molecule {i} has {n} atoms and {row.size} feature bytes')
            fp[n0:n0 + n] = row
        n0 += n
    dev = torch.device(device)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    return _pack(fn, torch.from_numpy(cls).to(dev).reshape(1, N), off, torch.from_numpy(pos).to(dev), 0,
                 torch.from_numpy(fp).to(dev).reshape(1, N) if fps is not None else None, None, len(sizes), 1, N, max(sizes, default=0), options)


@torch.no_grad()
def from_molecules(mols, device, options=ShapeOptions()):
    """The set of assembled molecules (`molecule.assemble`: 'element', 'atom_pos') on `device`, one row each: the counterpart of
    `similarity.stack`.  The set has colour iff every molecule carries m['features']['atom_fp'] (`assemble(features=)`).  A row's
    values are bit-identical to those of the same molecule in `shape_set`."""
    colour = len(mols) > 0 and all('features' in m and 'atom_fp' in m['features'] for m in mols)
    return _from_arrays('from_molecules', [list(m['element']) for m in mols], [np.asarray(m['atom_pos']) for m in mols],
                        [m['features']['atom_fp'] for m in mols] if colour else None, device, options)


def read_mol_block(text):
    """(atomic numbers, float32 [n, 3]) of the heavy atoms of a V2000 mol block, in the block's order.  Hydrogens are skipped; an
    element outside ATOM_TYPES raises ValueError.  Host only."""
    lines = text.split('\n')
    if len(lines) < 4 or 'V2000' not in lines[3]:
        raise ValueError('phoregen_amd.shape.from_mol_block: not a V2000 mol block (no counts line)')
    try:
        na = int(lines[3][0:3])
        rows = [(ln[31:34].strip(), float(ln[0:10]), float(ln[10:20]), float(ln[20:30])) for ln in lines[4:4 + na]]
    except ValueError as err:
        raise ValueError(f'phoregen_amd.shape.from_mol_block: malformed atom block ({err})') from None
    if len(rows) != na:
        raise ValueError(f'phoregen_amd.shape.from_mol_block: the counts line announces {na} atoms, the block has {len(rows)}')
    elements, pos = [], []
    for sym, x, y, z in rows:
        if sym in ('H', 'D', 'T'):
            continue
        if sym not in _SYMBOL_Z:
            raise ValueError(f'phoregen_amd.shape.from_mol_block: element {sym!r} is none of {sorted(_SYMBOL_Z)}')
        elements.append(_SYMBOL_Z[sym]), pos.append((x, y, z))
    return elements, np.asarray(pos, dtype=np.float32).reshape(-1, 3)


@torch.no_grad()
def from_mol_block(text, device, options=ShapeOptions()):
    """A one-row set from a V2000 mol block (`read_mol_block`), typically the reference ligand the pharmacophore was derived from, in
    the pharmacophore's frame.  Hydrogens are skipped; an element outside ATOM_TYPES raises ValueError.  The row carries no colour."""
    elements, pos = read_mol_block(text)
    return _from_arrays('from_mol_block', [elements], [pos], None, device, options)


def select_rows(s, index):
    """The rows `index` (a long tensor or a list) of a set as a set of their own, in that order; the atoms are shared."""
    index = torch.as_tensor(index, dtype=torch.long, device=s.mol.device).reshape(-1)
    return ShapeSet(atoms=s.atoms, mol=s.mol[index].contiguous(), status=s.status[index].contiguous(),
                    self_shape=s.self_shape[index].contiguous(), self_colour=s.self_colour[index].contiguous(), has_colour=s.has_colour,
                    options=s.options)


def concat(sets):
    """One set of the rows of `sets` in order; they must share their options and device.  It has colour iff every set has."""
    sets = list(sets)
    if not sets:
        raise ValueError('phoregen_amd.shape.concat: no set')
    for s in sets:
        if not isinstance(s, ShapeSet) or s.options != sets[0].options or s.atoms.device != sets[0].atoms.device:
            raise ValueError('phoregen_amd.shape.concat: the sets must be ShapeSets of the same options on one device')
    colour = all(s.has_colour for s in sets)
    mols, a0 = [], 0
    for s in sets:
        m = s.mol.clone()
        m[:, 0] += a0
        mols.append(m)
        a0 += s.atoms.size(0)
    zeros = lambda s: torch.zeros_like(s.self_colour)              # noqa: E731
    return ShapeSet(atoms=torch.cat([s.atoms for s in sets]), mol=torch.cat(mols), status=torch.cat([s.status for s in sets]),
                    self_shape=torch.cat([s.self_shape for s in sets]),
                    self_colour=torch.cat([s.self_colour if colour else zeros(s) for s in sets]), has_colour=colour, options=sets[0].options)


@dataclass
class ShapeSimilarity:
    """Device tensors of one `similarity` call."""
    shape: torch.Tensor          # fp32 [na, nb] ST
    colour: torch.Tensor         # fp32 [na, nb] CT; None when either set has no colour


def _check_set(fn, s, what):
    if not isinstance(s, ShapeSet):
        raise ValueError(f'phoregen_amd.shape.{fn}: {what} must be a ShapeSet, not {type(s).__name__}')
    _need_cuda(fn, s.atoms.device)
    for name, t, dt, tail in (('atoms', s.atoms, torch.float32, (4,)), ('mol', s.mol, torch.int32, (2,)), ('status', s.status, torch.int32, ()),
                              ('self_shape', s.self_shape, torch.float32, ()), ('self_colour', s.self_colour, torch.float32, ())):
        if (not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape[1:]) != tail or not t.is_contiguous() or t.device != s.atoms.device
                or (name not in ('atoms',) and t.size(0) != s.mol.size(0))):
            raise ValueError(f'phoregen_amd.shape.{fn}: {what}.{name} must be a contiguous {dt} tensor [n{"".join(", %d" % k for k in tail)}] '
                             f'on {s.atoms.device}')
    if s.atoms.size(0) > 0x7fffffff or s.n > 0x7fffffff:
        raise ValueError(f'phoregen_amd.shape.{fn}: {what} has {s.n} rows and {s.atoms.size(0)} atom rows, at most 2**31 - 1')


def _pair(fn, a, b):
    _check_set(fn, a, 'a')
    if b is not None:
        _check_set(fn, b, 'b')
        if b.atoms.device != a.atoms.device:
            raise ValueError(f'phoregen_amd.shape.{fn}: a lives on {a.atoms.device}, b on {b.atoms.device}')
        if b.options != a.options:
            raise ValueError(f'phoregen_amd.shape.{fn}: a and b were packed with different options ({a.options}, {b.options})')


@torch.no_grad()
def similarity(a, b=None):
    """ST, and CT where both sets have colour, of every row of a to every row of b (b=None: of a): fp32 [na, nb] each on the device
    (pg_shape_similarity).  na * nb is at most 2**31 - 1; `nearest` needs no matrix."""
    _pair('similarity', a, b)
    b = a if b is None else b
    na, nb = a.n, b.n
    if na * nb > 0x7fffffff:
        raise ValueError(f'phoregen_amd.shape.similarity: {na} x {nb} elements exceed 2**31 - 1; use nearest(), or cut the sets')
    dev = a.atoms.device
    colour = a.has_colour and b.has_colour
    with torch.cuda.device(dev):
        lib = hip.lib()
        st = torch.empty(na, nb, dtype=torch.float32, device=dev)
        ct = torch.empty(na, nb, dtype=torch.float32, device=dev) if colour else None
        _launch_similarity(lib, a, b, _alpha_arg(a.options), st, ct)
    return ShapeSimilarity(shape=st, colour=ct)


def _check_weight(fn, w):
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
        raise ValueError(f'phoregen_amd.shape.{fn}: colour_weight must be a number in [0, 1], not {w!r}')
    return float(w)


@torch.no_grad()
def nearest(a, b=None, colour_weight=0.0):
    """For every row of a its nearest neighbour among the rows of b by the score (1 - colour_weight) ST + colour_weight CT
    (pg_shape_nearest): the largest score, the lowest row that attains it, and the fp64 sum of the row's fp32 scores.  b=None: among the
    other rows of a (row i itself is left out).  CT is 0 where either set has no colour.  An empty row of b scores 0 and is still a
    candidate; a row without a candidate has similarity -1, index -1, sum 0.  No matrix, no host synchronisation."""
    w = _check_weight('nearest', colour_weight)
    _pair('nearest', a, b)
    same = b is None
    b = a if same else b
    dev = a.atoms.device
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = Nearest(sim=torch.empty(a.n, dtype=torch.float32, device=dev), index=torch.empty(a.n, dtype=torch.int32, device=dev),
                      sum=torch.empty(a.n, dtype=torch.float64, device=dev))
        _launch_nearest(lib, a, b, same, a.has_colour and b.has_colour, w, _alpha_arg(a.options), out)
    return out


@torch.no_grad()
def internal_diversity(a, colour_weight=0.0):
    """One minus the mean score of the distinct pairs of the rows of a that are not empty: with m such rows (status 0),
    1 - sum_i nearest(a).sum[i] / (m (m - 1)), the sum over those rows only; nan for m < 2.  An empty row scores exactly 0 against
    every row, so it adds nothing to the sum of another row, and leaving its own row out of the sum and itself out of m leaves it out
    altogether.  One host read."""
    _check_set('internal_diversity', a, 'a')
    live = a.status == 0
    near = nearest(a, colour_weight=colour_weight)
    total, m = torch.stack([torch.where(live, near.sum, torch.zeros_like(near.sum)).sum(), live.sum().double()]).tolist()
    return _diversity(total, int(m))


# ---- rigid overlay (csrc/shape_align.hip; DESIGN.md 2.9 "Shape alignment") -------------------------------------------------------------
START_NAMES = ('in_place', 'inertial', 'both')
_START_MASK = {'in_place': hip.PG_SHAPE_ALIGN_IN_PLACE, 'inertial': hip.PG_SHAPE_ALIGN_INERTIAL,
               'both': hip.PG_SHAPE_ALIGN_IN_PLACE | hip.PG_SHAPE_ALIGN_INERTIAL}


@dataclass(frozen=True)
class AlignOptions:
    """The step rule of `align`: at most max_steps evaluations per start (1 .. 1024, the first counts), steps from first_step down to
    min_step (Angstrom of the six-vector (translation, rho * rotation)), and the starts: 'in_place' (start 0), 'inertial' (starts
    1 .. 4, the four proper sign choices of the principal axes) or 'both'."""
    max_steps: int = 128
    first_step: float = 0.5
    min_step: float = 1e-4
    starts: str = 'both'

    def mask(self):
        if self.starts not in _START_MASK:
            raise ValueError(f'phoregen_amd.shape.AlignOptions: starts must be one of {START_NAMES}, not {self.starts!r}')
        return _START_MASK[self.starts]


@dataclass
class ShapeAlignment:
    """Device tensors of one `align` call, one row per pair."""
    pairs: torch.Tensor            # int32 [n, 2] row of a, row of b
    shape_overlap: torch.Tensor    # fp32  [n] V(A, B') at the winning pose
    colour_overlap: torch.Tensor   # fp32  [n] C(A, B'); 0 without colour or with colour_weight 0
    shape: torch.Tensor            # fp32  [n] ST
    colour: torch.Tensor           # fp32  [n] CT
    score: torch.Tensor            # fp32  [n] (1 - w) ST + w CT
    rotation: torch.Tensor         # fp32  [n, 3, 3] R ...
    translation: torch.Tensor      # fp32  [n, 3]    ... and t: y' = R y + t on b's stored coordinates
    start: torch.Tensor            # int32 [n] the winning start, 0 in place, 1 .. 4 inertial; -1 for a pair with an empty row
    steps: torch.Tensor            # int32 [n] the evaluations the winning start used


def _launch_frames(lib, s, out):
    """pg_shape_frames on the current stream."""
    hip.check(lib.pg_shape_frames(s.atoms.data_ptr(), s.atoms.size(0), s.mol.data_ptr(), s.n, out.data_ptr(), hip.stream_ptr()), 'pg_shape_frames')


def _align_args(s, frames_):
    return (s.atoms.data_ptr(), s.atoms.size(0), s.mol.data_ptr(), s.self_shape.data_ptr(), s.self_colour.data_ptr(), frames_.data_ptr(), s.n)


def _launch_align(lib, a, fa, b, fb, pairs, n_pairs, has_colour, w, alpha, max_steps, first_step, min_step, mask, values, transform, start, steps):
    """pg_shape_align on the current stream; pairs may be None (the grid a x b).  Bad options, a bad weight or alpha and a listed pair
    outside its set are the library's errors: nothing is launched and the outputs are not written."""
    hip.check(lib.pg_shape_align(*_align_args(a, fa), *_align_args(b, fb), hip.ptr(pairs), n_pairs, int(has_colour), w, alpha, max_steps,
                                 first_step, min_step, mask, values.data_ptr(), transform.data_ptr(), start.data_ptr(), steps.data_ptr(),
                                 hip.stream_ptr()), 'pg_shape_align')


@torch.no_grad()
def frames(s):
    """The frame of every row of a set, fp32 [n, 16] on the device (pg_shape_frames): centroid 3, principal axes 9 (axis k at
    3 + 3 k, eigenvalues descending, right-handed), rho = max(radius of gyration, 0.5), the three eigenvalues of the covariance.
    Computed in double, rounded once.  An empty row: the origin, the identity, rho 0.5."""
    _check_set('frames', s, 's')
    dev = s.atoms.device
    with torch.cuda.device(dev):
        out = torch.empty(s.n, hip.PG_SHAPE_FRAME_FLOATS, dtype=torch.float32, device=dev)
        _launch_frames(hip.lib(), s, out)
    return out


@torch.no_grad()
def align(a, b=None, pairs=None, colour_weight=0.0, options=AlignOptions()):
    """The best rigid overlay of b's row onto a's row for every pair (pg_shape_frames, pg_shape_align): a stays, b moves; from each
    enabled start a fixed-rule gradient ascent of the score (1 - colour_weight) ST + colour_weight CT, the best final score winning, ties
    to the lowest start.  pairs: int32 [n, 2] on the device (row of a, row of b; read back once to be checked), default the grid
    a x b in row-major order, built on the device with no host read.  b=None: a against itself.  With colour_weight 0 or a set without
    colour, CT and the colour overlap are 0.  A pair's values are bit-identical wherever it stands in the list.  The scores are this
    module's, not ROCS's or RDKit's."""
    w = _check_weight('align', colour_weight)
    _pair('align', a, b)
    b = a if b is None else b
    if not isinstance(options, AlignOptions):
        raise ValueError(f'phoregen_amd.shape.align: options must be an AlignOptions, not {options!r}')
    mask = options.mask()
    dev = a.atoms.device
    if pairs is not None:
        if not torch.is_tensor(pairs) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.size(1) != 2 or pairs.device != dev:
            raise ValueError(f'phoregen_amd.shape.align: pairs must be an int32 tensor [n, 2] on {dev}')
        pairs = pairs.contiguous()
        n = pairs.size(0)
    else:
        n = a.n * b.n
    if n > 0x7fffffff:
        raise ValueError(f'phoregen_amd.shape.align: {n} pairs exceed 2**31 - 1; cut the sets')
    with torch.cuda.device(dev):
        lib = hip.lib()
        fa = frames(a)
        fb = fa if b is a else frames(b)
        values = torch.empty(n, 5, dtype=torch.float32, device=dev)
        transform = torch.empty(n, 12, dtype=torch.float32, device=dev)
        start = torch.empty(n, dtype=torch.int32, device=dev)
        steps = torch.empty(n, dtype=torch.int32, device=dev)
        _launch_align(lib, a, fa, b, fb, pairs, n, a.has_colour and b.has_colour, w, _alpha_arg(a.options), int(options.max_steps),
                      float(options.first_step), float(options.min_step), mask, values, transform, start, steps)
        if pairs is None:
            pairs = torch.cartesian_prod(torch.arange(a.n, dtype=torch.int32, device=dev),
                                         torch.arange(b.n, dtype=torch.int32, device=dev)).reshape(-1, 2)
    return ShapeAlignment(pairs=pairs, shape_overlap=values[:, 0], colour_overlap=values[:, 1], shape=values[:, 2], colour=values[:, 3],
                          score=values[:, 4], rotation=transform[:, :9].reshape(n, 3, 3), translation=transform[:, 9:], start=start, steps=steps)


@torch.no_grad()
def transformed(s, rows, rotation, translation):
    """The rows `rows` of a set moved by the given transforms, as a set of their own in that order: row k's atoms at R_k y + t_k (torch
    on the device, fp32), the feature words kept, the self overlaps copied -- a rigid move does not change them.  rotation [n, 3, 3],
    translation [n, 3], e.g. `ShapeAlignment.rotation` / `.translation` with rows = pairs[:, 1]."""
    _check_set('transformed', s, 's')
    dev = s.atoms.device
    rows = torch.as_tensor(rows, dtype=torch.long, device=dev).reshape(-1)
    n = rows.numel()
    if (not torch.is_tensor(rotation) or not torch.is_tensor(translation) or tuple(rotation.shape) != (n, 3, 3) or tuple(translation.shape) != (n, 3)
            or rotation.dtype != torch.float32 or translation.dtype != torch.float32 or rotation.device != dev or translation.device != dev):
        raise ValueError(f'phoregen_amd.shape.transformed: rotation must be fp32 [{n}, 3, 3] and translation fp32 [{n}, 3] on {dev}')
    mol = s.mol[rows]
    count = mol[:, 1].long()
    first = torch.cumsum(count, 0) - count
    owner = torch.repeat_interleave(torch.arange(n, device=dev), count)
    src = mol[:, 0].long()[owner] + (torch.arange(owner.numel(), device=dev) - first[owner])
    atoms = s.atoms[src].clone()
    atoms[:, :3] = torch.einsum('nij,nj->ni', rotation[owner], atoms[:, :3]) + translation[owner]
    return ShapeSet(atoms=atoms, mol=torch.stack([first, count], 1).to(torch.int32).contiguous(), status=s.status[rows].contiguous(),
                    self_shape=s.self_shape[rows].contiguous(), self_colour=s.self_colour[rows].contiguous(), has_colour=s.has_colour,
                    options=s.options)
