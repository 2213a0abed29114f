"""3D hydrogens on the device (csrc/mol_hydrogens.hip, csrc/hydrogen_core.h; DESIGN.md 2.9 "Hydrogens"): every hydrogen `kekulize`
counted gets coordinates, so that the pipeline ends at an all-atom structure.

`hydrogens` places, for every decoded (frame, graph) in one launch, the hydrogens of every kept atom from the ideal local geometry of
that atom alone: its shape (tetrahedral, trigonal, linear) follows from the Kekulé orders by an integer rule, the directions from the
unit vectors to its heavy neighbours, the distance from `XH_LENGTH`.  It also counts the contacts the new hydrogens make -- a hydrogen
closer than `clash_min` to an atom other than its parent or to a hydrogen of another parent.  `all_atoms` lists heavy atoms and
hydrogens of an assembled molecule; `molecule.assemble(hydrogens=)`, `molecule.sample_valid(hydrogens=)`, `molecule.mol_block` (an
all-atom block) and `molecule.write_sdf` carry the answers.

Necessary, not sufficient, in the project's usual sense: ideal local geometry only -- no force field, no rotor search, no hydrogen-bond
network, no look at anything beyond the neighbour's neighbour; a methyl or hydroxyl torsion is the staggered one by the numbering rule,
not the best one.  `XH_LENGTH`, `clash_min` and the degeneracy threshold are design choices written from memory; nothing here was
checked against RDKit or OpenBabel."""
from dataclasses import dataclass

import numpy as np
import torch

from . import hip
from . import molecule as M
from .utils.sample_utils import ATOM_TYPES

MAX_PER_ATOM = hip.PG_HYD_MAX_PER_ATOM       # hydrogen slots of an atom row
DEG_EPS = hip.PG_HYD_DEG_EPS                 # a vector of unit inputs with a norm below this has no direction (a design choice)

HYD_NO_KEKULE = 1                # the graph's Kekulé status has KEKULE_FAILED: no hydrogen counts to place
HYD_NONFINITE = 2                # a kept atom with a non-finite coordinate: nothing is placed at it or next to it
HYD_TOO_MANY = 4                 # a kept atom with more than MAX_PER_ATOM hydrogens: nothing is placed in the graph
HYD_CONTACTS = 8                 # more than max_contacts contacts
HYD_GENERIC = 16                 # informational: at least one site was placed by the generic rule
HYD_HAS_HYDROGEN = 32            # informational: at least one hydrogen was placed
HYD_FAIL_MASK = HYD_NO_KEKULE | HYD_NONFINITE | HYD_TOO_MANY | HYD_CONTACTS
HYD_NAMES = {HYD_NO_KEKULE: 'NO_KEKULE', HYD_NONFINITE: 'NONFINITE', HYD_TOO_MANY: 'TOO_MANY', HYD_CONTACTS: 'CONTACTS',
             HYD_GENERIC: 'GENERIC', HYD_HAS_HYDROGEN: 'HAS_HYDROGEN'}
HYD_COUNTS = ('hydrogens', 'sites', 'sites_tetrahedral', 'sites_trigonal', 'sites_linear', 'sites_generic', 'contacts', 'kept_atoms')
SHAPE_NONE, SHAPE_TETRAHEDRAL, SHAPE_TRIGONAL, SHAPE_LINEAR, SHAPE_GENERIC = range(5)
SHAPE_NAMES = ('none', 'tetrahedral', 'trigonal', 'linear', 'generic')

# X-H distance in Angstrom by atomic number.  Design choices written from memory (typical X-H lengths of small molecules), NOT checked
# against any toolkit.  This is the only copy: the kernel and the tests' restatement are handed the table.
XH_LENGTH = {5: 1.19, 6: 1.09, 7: 1.01, 8: 0.96, 9: 0.92, 14: 1.48, 15: 1.42, 16: 1.34, 17: 1.27, 35: 1.41, 53: 1.61}


@dataclass(frozen=True)
class HydrogenOptions:
    """xh_length: the X-H distance per atom class in Angstrom, eleven numbers in ATOM_TYPES order (default: `XH_LENGTH`); clash_min: a
    hydrogen closer than this to an atom other than its parent, or to a hydrogen of another parent, is a contact (strict, fp32; 1.5 is
    a design choice: well below every 1-3 distance of an ideal geometry, above an X-H bond); max_contacts: HYD_CONTACTS is set when a
    graph has more contacts than this.  With the defaults only HYD_NO_KEKULE / HYD_NONFINITE / HYD_TOO_MANY can fail;
    HydrogenOptions(max_contacts=0) asks for a contact-free placement."""
    xh_length: tuple = tuple(XH_LENGTH[z] for z in ATOM_TYPES)
    clash_min: float = 1.5
    max_contacts: int = 2 ** 31 - 1

    def __post_init__(self):
        xh = self.xh_length
        if isinstance(xh, (str, bytes)) or not hasattr(xh, '__len__') or len(xh) != len(ATOM_TYPES):
            raise ValueError(f'HydrogenOptions: xh_length must hold {len(ATOM_TYPES)} numbers in ATOM_TYPES order, not {xh!r}')
        for z, v in zip(ATOM_TYPES, xh):
            M._check_number('HydrogenOptions', f'xh_length[{M.ELEMENT_SYMBOL[z]}]', v, False)
        object.__setattr__(self, 'xh_length', tuple(float(v) for v in xh))
        M._check_number('HydrogenOptions', 'clash_min', self.clash_min, False)
        M._check_int('HydrogenOptions', 'max_contacts', self.max_contacts, 0, 0x7fffffff)


@dataclass
class Hydrogens:
    """Device tensors of one `hydrogens` call; F frames, B graphs, N atom rows."""
    status: torch.Tensor         # int32 [F, B]        HYD_* bits
    counts: torch.Tensor         # int32 [F, B, 8]     HYD_COUNTS
    ok: torch.Tensor             # bool  [F, B]        no bit of HYD_FAIL_MASK
    h_pos: torch.Tensor          # fp32  [F, N, 4, 3]  the hydrogens of the atom row, slot by slot; unused slots 0
    h_placed: torch.Tensor       # uint8 [F, N]        hydrogens placed at the atom: 0 or its hcount
    site_shape: torch.Tensor     # uint8 [F, N]        SHAPE_* of the rule that placed them, 0 = no site
    min_contact: torch.Tensor    # fp32  [F, B]        the smallest contact distance, +inf without a pair (0 with HYD_NO_KEKULE)
    options: HydrogenOptions
    screen: M.Screen             # the screen and the Kekulé form it was computed from
    kekule: M.Kekule


def _length_table(options, device):
    """options.xh_length as fp32 [11] on `device` (eleven floats, uploaded per call: nothing is kept)."""
    return torch.tensor(options.xh_length, dtype=torch.float32, device=device)


@torch.no_grad()
def hydrogens(results, frames='final', screen=None, kekule=None, options=HydrogenOptions()):
    """Coordinates for the hydrogens of every decoded (frame, graph) of a `sample` / `sample_batch` result, on the device, in one
    launch (pg_mol_hydrogens; DESIGN.md 2.9 "Hydrogens").  Whichever of `screen` and `kekule` (a `Kekule`) is not handed in is
    computed; both must come from one screen.  No host read beyond the screen's.  The output is dense: four slots per atom row, so a
    graph's hydrogens are where its atoms are and nothing needs a prefix sum.  `ok` fails without a Kekulé structure, with a
    non-finite coordinate, with more than four hydrogens on an atom, or with more than options.max_contacts contacts.  Ideal local
    geometry only; the lengths and thresholds are design choices; not checked against RDKit / OpenBabel."""
    node, pos, _, F, (_, _, pos_fs) = M._frames(results, frames)
    dev = pos.device
    M._need_cuda('hydrogens', 'the hydrogen placement', dev)
    if not isinstance(options, HydrogenOptions):
        raise ValueError(f'phoregen_amd.hydrogens.hydrogens: options must be a HydrogenOptions, not {options!r}')
    if kekule is not None and not isinstance(kekule, M.Kekule):
        raise ValueError(f'phoregen_amd.hydrogens.hydrogens: kekule= must be a Kekule, not {kekule!r}')
    sc = M._resolve('hydrogens', results, frames, screen, 'phoregen_amd.hydrogens', kekule=kekule)
    M._check_rows('hydrogens', pos, F, 3, 'coordinates', dev)
    kek = kekule if kekule is not None else M.kekulize(results, frames, screen=sc)
    B, N = len(sc.num_atoms), pos.size(-2)
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(HYD_COUNTS), dtype=torch.int32, device=dev),
                   h_pos=torch.empty(F, N, MAX_PER_ATOM, 3, dtype=torch.float32, device=dev),
                   h_placed=torch.empty(F, N, dtype=torch.uint8, device=dev), site_shape=torch.empty(F, N, dtype=torch.uint8, device=dev),
                   min_contact=torch.empty(F, B, dtype=torch.float32, device=dev))
        _launch_hydrogens(lib, pos, pos_fs, sc, kek, B, F, max(sc.num_atoms, default=0), _length_table(options, dev), options, out)
    return Hydrogens(ok=(out['status'] & HYD_FAIL_MASK) == 0, options=options, screen=sc, kekule=kek, **out)


def _launch_hydrogens(lib, pos, pos_fs, sc, kek, B, F, max_n, table, options, out):
    """pg_mol_hydrogens on the current stream; sc, kek: anything with the `Screen` and `Kekule` fields the kernel reads; table: fp32 [11]
    on the device.  A graph above MAX_ATOMS or an option out of range is the library's error: nothing is launched and `out` is not
    written."""
    cls, order = sc.cls, sc.order
    M._check_arrays('hydrogens', pos.device, [
        (cls, torch.int8), (order, torch.int8), (kek.kekule_order, torch.int8), (kek.hcount, torch.uint8), (kek.charge, torch.int8),
        (kek.status, torch.int32), (sc.lig_off, torch.int32), (sc.bond_off, torch.int32), (table, torch.float32),
        (out['h_pos'], torch.float32), (out['h_placed'], torch.uint8), (out['site_shape'], torch.uint8), (out['min_contact'], torch.float32),
        (out['counts'], torch.int32), (out['status'], torch.int32)])
    if (sc.lig_off.numel() != B + 1 or sc.bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or pos.size(-2) != cls.size(-1) or pos.dtype != torch.float32 or pos.device != cls.device
            or kek.hcount.shape != cls.shape or kek.charge.shape != cls.shape or kek.kekule_order.shape != order.shape
            or kek.status.numel() != F * B or table.numel() != len(ATOM_TYPES)
            or out['h_pos'].numel() != 3 * MAX_PER_ATOM * cls.numel() or out['h_placed'].shape != cls.shape
            or out['site_shape'].shape != cls.shape or out['min_contact'].numel() != F * B or out['status'].numel() != F * B
            or out['counts'].numel() != len(HYD_COUNTS) * F * B):
        raise ValueError('phoregen_amd.hydrogens.hydrogens: sizes of the offsets, screen / Kekulé arrays, table and outputs do not fit '
                         f'{F} frames x {B} graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_hydrogens(pos.data_ptr(), pos_fs, cls.data_ptr(), order.data_ptr(), kek.kekule_order.data_ptr(),
                                   kek.hcount.data_ptr(), kek.charge.data_ptr(), kek.status.data_ptr(), sc.lig_off.data_ptr(),
                                   sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1), max_n, table.data_ptr(),
                                   float(options.clash_min), int(options.max_contacts), out['h_pos'].data_ptr(),
                                   out['h_placed'].data_ptr(), out['site_shape'].data_ptr(), out['min_contact'].data_ptr(),
                                   out['counts'].data_ptr(), out['status'].data_ptr(), hip.stream_ptr()), 'pg_mol_hydrogens')


def status_names(status):
    return tuple(name for bit, name in HYD_NAMES.items() if status & bit)


def molecule_entry(status, counts, min_contact, h_pos, h_placed, site_shape):
    """The 'hydrogens' dict of one assembled molecule from the graph's rows restricted to its kept atoms: h_pos [n, 4, 3], h_placed
    and site_shape [n]; hydrogens in (parent, slot) order, parents as indices into the molecule's atoms."""
    placed = np.asarray(h_placed).astype(np.int64)
    parent = np.repeat(np.arange(placed.size, dtype=np.int64), placed)
    slot = np.concatenate([np.arange(k, dtype=np.int64) for k in placed.tolist()]) if parent.size else np.zeros(0, dtype=np.int64)
    return dict({'status': int(status), 'hydrogens_ok': (int(status) & HYD_FAIL_MASK) == 0},
                **{k: int(x) for k, x in zip(HYD_COUNTS, counts)}, min_contact=float(min_contact),
                h_pos=np.asarray(h_pos, dtype=np.float32).reshape(-1, MAX_PER_ATOM, 3)[parent, slot].copy(), h_parent=parent,
                site_shape=np.asarray(site_shape).astype(np.uint8).copy())


def all_atoms(mol):
    """(elements, positions float64 [n, 3]) of an assembled molecule, heavy atoms first and then, if it carries 'hydrogens' with
    'hydrogens_ok', its hydrogens (atomic number 1) in (parent, slot) order."""
    elements = [int(z) for z in mol['element']]
    pos = np.asarray(mol['atom_pos'], dtype=np.float64).reshape(-1, 3)
    hy = mol.get('hydrogens')
    if hy is not None and hy.get('hydrogens_ok'):
        h_pos = np.asarray(hy['h_pos'], dtype=np.float64).reshape(-1, 3)
        elements, pos = elements + [1] * len(h_pos), np.concatenate([pos, h_pos])
    return elements, pos


def sdf_item(hy):
    """The PHOREGEN_HYDROGENS data item of a molecule's 'hydrogens' dict (`molecule.write_sdf`)."""
    mc = hy['min_contact']
    return ('> <PHOREGEN_HYDROGENS>\nstatus 0x%02x\n' % int(hy['status']) + ''.join('%s %d\n' % (k, hy[k]) for k in HYD_COUNTS)
            + 'min_contact %s\n\n' % ('%.4f' % mc if np.isfinite(mc) else 'inf'))


# What `molecule.assemble`, `write_sdf` and `sample_valid` know about this analysis.  An all-atom block needs the Kekulé form: `also`.
ANALYSIS = M._Analysis(
    'hydrogens', 'hydrogens', Hydrogens, also=('kekule',),
    parts=lambda x: [('h_status', x.status[0], np.int32), ('h_counts', x.counts[0], np.int32), ('h_min', x.min_contact[0], np.float32),
                     ('h_pos', x.h_pos[0], np.float32), ('h_placed', x.h_placed[0], np.uint8), ('h_shape', x.site_shape[0], np.uint8)],
    entry=lambda x, v, at, mol: {'hydrogens': molecule_entry(at.row(v['h_status']), at.row(v['h_counts']), at.row(v['h_min']),
                                                             at.atoms(v['h_pos']), at.atoms(v['h_placed']), at.atoms(v['h_shape']))},
    sdf=lambda m: sdf_item(m['hydrogens']), read=lambda value: None if value is False else M._true_or('hydrogens', HydrogenOptions)(value),
    compute=lambda d, opt: hydrogens(d.res, screen=d.screen, kekule=d.of('kekule'), options=opt),
    verdict=lambda m: m['hydrogens']['hydrogens_ok'])
