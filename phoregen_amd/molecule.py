"""From sampler output to molecules (beyond the reference's library code; its driver does this with RDKit, sample_all.py:79-175).

`screen` answers, on the device and for every (frame, graph) in one launch (csrc/mol_screen.hip), the two questions the top-up loop
of sample_all.py needs: is this ONE molecule, and can these atoms carry these bonds.  `assemble` turns the final prediction into
per-molecule arrays with `decode_data`'s keys, `mol_block` / `write_sdf` write them as V2000 mol blocks, `sample_valid` is the loop
that samples until enough molecules have passed.  No RDKit, no OpenBabel: `valid` is necessary, not sufficient, for the reference's
`Chem.SanitizeMol` (DESIGN.md "From sampler output to molecules").

Identity: `molecule_keys` gives every decoded molecule a 64-bit key that does not depend on the numbering of its atoms
(csrc/mol_key.hip; the definition is in DESIGN.md 2.9 "Identity"), `same_molecule` decides exactly whether two assembled molecules
have the same atoms and bonds, `unique_molecules` / `duplicate_groups` / `sample_valid(unique=True)` use the two.  Equal keys are
necessary, not sufficient, for equal molecules; this is not SMILES.  The key is constitution only: two enantiomers, or a cis and a
trans isomer, share it; `stereo`'s `stereo_key` and the `stereo=True` forms of these functions tell them apart.

Geometry: `geometry` / `geometry_for` measure the decoded molecules where they lie (csrc/mol_geom.hip; DESIGN.md 2.9 "Geometry"):
bond lengths, non-bonded clashes, clearance from the exclusion spheres, which feature points have an atom nearby, and the reference's
two guidance energies on the decoded molecule.  `assemble(geometry=)`, `sample_valid(geometry=)` and `write_sdf` carry it.  Again
necessary, not sufficient: no force field, no hydrogens, no feature typing.

Rings: `rings` finds the smallest ring through every bond and atom, the ring systems and the counts users filter on (csrc/mol_rings.hip;
DESIGN.md 2.9 "Rings"): three- and four-membered rings, macrocycles, oversized fused systems, aromatic bonds outside a ring, rotatable
bonds.  `assemble(rings=)`, `sample_valid(rings=)` and `write_sdf` carry it.  Exact integer answers; no kekulisation, no ring list.

Kekulé form: `kekulize` resolves the aromatic bond class into single and double bonds and gives every atom its hydrogens and its
charge (csrc/mol_kekule.hip; DESIGN.md 2.9 "Kekulé form"): an exact matching on the aromatic bonds, neutral first, with N+ / P+ / S+
if that is allowed and needed.  `assemble(kekule=)`, `sample_valid(kekule=)`, `mol_block` and `write_sdf` carry it.  Which Kekulé
structure is returned is not canonical; not checked against RDKit.

Features: `features` / `features_for` give every atom the pharmacophore feature types it presents -- the reference's SMARTS for HD, AR,
PO, HA, HY, NE, XB restated as integer rules over the Kekulé form, the hydrogens, the charges and the ring membership -- and match
every typed feature point against the atoms that carry its type (csrc/mol_feat.hip; DESIGN.md 2.9 "Features"), as the reference's
`check_nearby_phore(strict=True)` does with RDKit.  `assemble(features=)`, `sample_valid(features=)` and `write_sdf` carry it.  MB, CV
and CR are not typed; the tables are written from the SMARTS text and not checked against RDKit.

SMILES: `smiles` writes every decoded molecule as Kekulé-form OpenSMILES text on the device (csrc/mol_smiles.hip; DESIGN.md 2.9
"SMILES"): a depth-first walk in atom order, ring-closure labels 1..99, bracket atoms where the bare symbol would not read back with
the atom's hydrogens and charge.  `Smiles.strings`, `assemble(smiles=)`, `sample_valid(smiles=)` and `write_sdf` carry it.  The text
reads back to exactly the molecule `assemble` returns; it is not canonical (identity stays with the keys), has no aromatic lower-case
form, and is not checked against RDKit.  Without `stereo=` it has no stereo.

Stereo: `stereo` reads from the coordinates which way round every tetrahedral centre is and whether every double bond outside a ring is
cis or trans (csrc/mol_stereo.hip; DESIGN.md 2.9 "Stereo"), gives each a label that does not depend on the numbering of the atoms, and
a `stereo_key` that tells stereoisomers apart where the identity key cannot.  `smiles(stereo=)` writes them into the text ('@', '@@',
'/', '\\': isomeric SMILES, csrc/mol_smiles.hip); `assemble(stereo=)`, `same_molecule(stereo=True)`, `unique_molecules(stereo=True)`,
`sample_valid(stereo=)` and `write_sdf` carry them.  No CIP names (R / S, E / Z), no pseudo-asymmetric centres, no ring double bonds,
allenes or atropisomers, no three-coordinate N, P or S; the two thresholds are design choices, not calibrated.

Fingerprints: `fingerprints` gives every decoded molecule a 2048-bit circular (Morgan-style) fingerprint (csrc/mol_fp.hip; DESIGN.md
2.9 "Fingerprints and similarity"): one bit per (atom, radius 0..R) environment identifier, built from the identity key's initial
colour and its `mix`, aromatic bonds as their own order.  `assemble(fingerprints=)`, `sample_valid(fingerprints=)` and `write_sdf` carry
it; `phoregen_amd.similarity` compares sets of them on the device (Tanimoto matrix, nearest neighbour, internal diversity, MaxMin
picks).  Exact and independent of the numbering of the atoms; NOT RDKit's ECFP (no duplicate-environment removal, other invariants,
another hash) and not checked against RDKit.

Distance bonds: `screen(bonds='distance')` perceives the bonds from the coordinates with the reference's `--add_edge distance` rule
(csrc/mol_screen_dist.hip; DESIGN.md 2.9 "Distance bonds") and returns the same `Screen`, so everything above works on them unchanged;
`bond_agreement` also counts how they agree with the predicted bonds.  `assemble(screen=)`, `sample_valid(add_edge=)` and `write_sdf`
carry it.  Orders 1..3 only: no aromatic order, no hydrogens, no `openbabel` mode.

Substructure: `phoregen_amd.substructure` answers whether, how often and where a decoded molecule contains a pattern (csrc/mol_sub.hip;
DESIGN.md 2.9 "Substructure"); `assemble(substructure=)`, `sample_valid(substructure=)` and `write_sdf` carry it.

Hydrogens: `phoregen_amd.hydrogens` gives every hydrogen `kekulize` counted its coordinates (csrc/mol_hydrogens.hip; DESIGN.md 2.9
"Hydrogens"): the shape of each site by an integer rule over the Kekulé orders, the directions from the unit vectors to its heavy
neighbours, and a count of the contacts the hydrogens make.  `assemble(hydrogens=)`, `sample_valid(hydrogens=)`, `mol_block` (an
all-atom block) and `write_sdf` carry it.  Ideal local geometry only: no force field, no rotor search; lengths and thresholds are
design choices, not checked against RDKit / OpenBabel.

Scaffolds: `phoregen_amd.scaffold` writes the Murcko scaffold of every decoded molecule as a `Screen` of its own
(csrc/mol_scaffold.hip; DESIGN.md 2.9 "Scaffolds"), so that `molecule_keys`, `fingerprints`, `kekulize`, `smiles` and
`assemble(screen=)` work on scaffolds unchanged, and groups molecules by scaffold.  It is a module of its own: `assemble`,
`sample_valid` and `write_sdf` do not carry it.

Properties: `phoregen_amd.properties` computes molecular weight, table sums (polar surface area, logP, molar refractivity), the
Lipinski and Veber counts, Fsp3 and a verdict against `PropertyLimits` (csrc/mol_props.hip; DESIGN.md 2.9 "Properties") from an
integer environment word per atom; `assemble(properties=)`, `sample_valid(properties=)` and `write_sdf` carry it.  The shipped
contribution tables are written from memory, not checked against RDKit; no QED, no synthetic-accessibility score.

Shape: `phoregen_amd.shape` compares molecules in space, where they lie in the pharmacophore's frame: Gaussian-volume shape overlap
and, with `Features.atom_fp`, feature ("colour") overlap, their Tanimoto values as an all-pairs matrix or a nearest-neighbour search,
and the 3D diversity of a run (csrc/shape_sim.hip; DESIGN.md 2.9 "Shape").  No alignment search, first order only, no hydrogens; the
radii are written from memory and the values are not ROCS's or RDKit's.  Like scaffolds it is a module of its own: `assemble`,
`sample_valid` and `write_sdf` do not carry it."""
import ctypes
from collections import namedtuple
from dataclasses import astuple, dataclass, replace
from functools import cached_property, lru_cache
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import torch

from . import hip
from .utils.sample_utils import ATOM_TYPES

STATUS_NO_ATOMS = 1              # nothing kept
STATUS_DISCONNECTED = 2          # more than one connected component (the heavy-atom equivalent of `'.' in smiles`)
STATUS_VALENCE = 4               # an atom above MAX_VALENCE (+ 1/2 if it has an aromatic bond)
STATUS_NONFINITE = 8             # a kept atom with a non-finite coordinate
STATUS_HAD_MASKED_ATOM = 16      # informational: an atom of class 11 was dropped
STATUS_HAD_ABSORBING_BOND = 32   # informational: a bond row (a < b) of class 5, read as "no bond"
FAIL_MASK = STATUS_NO_ATOMS | STATUS_DISCONNECTED | STATUS_VALENCE | STATUS_NONFINITE
STATUS_NAMES = {STATUS_NO_ATOMS: 'NO_ATOMS', STATUS_DISCONNECTED: 'DISCONNECTED', STATUS_VALENCE: 'VALENCE',
                STATUS_NONFINITE: 'NONFINITE', STATUS_HAD_MASKED_ATOM: 'HAD_MASKED_ATOM',
                STATUS_HAD_ABSORBING_BOND: 'HAD_ABSORBING_BOND'}

# `screen(bonds='distance')` only (DESIGN.md 2.9 "Distance bonds"; kept out of STATUS_NAMES / FAIL_MASK, which describe pg_mol_screen)
STATUS_DIST_UNMAPPED_ELEMENT = 64  # informational: a kept B or Si atom, for which the reference's `predict_bonds` raises KeyError
DISTANCE_STATUS_NAMES = {**{b: n for b, n in STATUS_NAMES.items() if b != STATUS_HAD_ABSORBING_BOND},
                         STATUS_DIST_UNMAPPED_ELEMENT: 'DIST_UNMAPPED_ELEMENT'}
BOND_MODES = ('predicted', 'distance')
# columns of `Screen.agree`: the pairs a < b of kept atoms with finite coordinates by (predicted order p, distance order o)
BOND_AGREE_COUNTS = ('both_same',        # p = o in 1..3
                     'both_aromatic',    # p = 4 and o in 1..2
                     'both_differ',      # both bonded, neither of the above
                     'predicted_only', 'distance_only', 'neither')

# Largest explicit valence an atom may carry, by atomic number: the largest entry of each element's default valence list as RDKit has
# it, with N raised to 4 because the reference turns a four-valent N into N+ instead of failing (utils/sample_utils.py:437-440).
# CAVEAT: written from memory; RDKit is not a dependency of this project and the table has not been checked against it.  The rule is
# one-sided on purpose: it must not reject what the reference's sanitisation would accept, and it accepts things RDKit rejects.
# This is the table's only copy: the kernel and the tests' restatement are handed it.
MAX_VALENCE = {5: 3, 6: 4, 7: 4, 8: 2, 9: 1, 14: 4, 15: 7, 16: 6, 17: 1, 35: 1, 53: 5}
assert list(MAX_VALENCE) == ATOM_TYPES

# Typical bond lengths in pm by element pair, in ATOM_TYPES order (B C N O F Si P S Cl Br I): single, double, triple; 0 = no entry.
# From the two public tables the reference's utils/predict_bonds.py cites (wiredchemist.com bond energies and lengths;
# chemistry-reference.com bond lengths and enthalpies), as that file's lookup (lower atomic number first) reads them: so C=S has its
# 160 although the table lists it from carbon's side only, fifteen pairs have no single-bond length and never bond (ten of boron's
# eleven -- only B-Cl has one -- and N-Si, Si-P, P-I, Cl-I, Br-I).  tests/test_molbonds_host.py pins every entry to values recorded
# from the reference.  This is the table's only copy: the kernel is handed `length + margin`, the tests' restatement reads this.
BOND_LENGTHS_PM = (
    (   # single
     #        B    C    N    O    F   Si    P    S   Cl   Br    I
        (  0,   0,   0,   0,   0,   0,   0,   0, 175,   0,   0),   # B
        (  0, 154, 147, 143, 135, 185, 184, 182, 177, 194, 214),   # C
        (  0, 147, 145, 140, 136,   0, 177, 168, 175, 214, 222),   # N
        (  0, 143, 140, 148, 142, 163, 163, 151, 164, 172, 194),   # O
        (  0, 135, 136, 142, 142, 160, 156, 158, 166, 178, 187),   # F
        (  0, 185,   0, 163, 160, 233,   0, 200, 202, 215, 243),   # Si
        (  0, 184, 177, 163, 156,   0, 221, 210, 203, 222,   0),   # P
        (  0, 182, 168, 151, 158, 200, 210, 204, 207, 225, 234),   # S
        (175, 177, 175, 164, 166, 202, 203, 207, 199, 214,   0),   # Cl
        (  0, 194, 214, 172, 178, 215, 222, 225, 214, 228,   0),   # Br
        (  0, 214, 222, 194, 187, 243,   0, 234,   0,   0, 266),   # I
    ),
    (   # double
     #        B    C    N    O    F   Si    P    S   Cl   Br    I
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # B
        (  0, 134, 129, 120,   0,   0,   0, 160,   0,   0,   0),   # C
        (  0, 129, 125, 121,   0,   0,   0,   0,   0,   0,   0),   # N
        (  0, 120, 121, 121,   0,   0, 150,   0,   0,   0,   0),   # O
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # F
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # Si
        (  0,   0,   0, 150,   0,   0,   0, 186,   0,   0,   0),   # P
        (  0, 160,   0,   0,   0,   0, 186,   0,   0,   0,   0),   # S
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # Cl
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # Br
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # I
    ),
    (   # triple
     #        B    C    N    O    F   Si    P    S   Cl   Br    I
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # B
        (  0, 120, 116, 113,   0,   0,   0,   0,   0,   0,   0),   # C
        (  0, 116, 110,   0,   0,   0,   0,   0,   0,   0,   0),   # N
        (  0, 113,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # O
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # F
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # Si
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # P
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # S
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # Cl
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # Br
        (  0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0),   # I
    ),
)
assert all(len(m) == len(ATOM_TYPES) and all(len(r) == len(ATOM_TYPES) for r in m) for m in BOND_LENGTHS_PM)
ELEMENT_SYMBOL = {5: 'B', 6: 'C', 7: 'N', 8: 'O', 9: 'F', 14: 'Si', 15: 'P', 16: 'S', 17: 'Cl', 35: 'Br', 53: 'I'}
MAX_ATOMS = hip.PG_MOL_MAX_ATOMS

# The identity key (DESIGN.md 2.9 "Identity"): constants of the splitmix64 step `mix`, the refinement rounds, the pair word of two
# atoms without a path between them, and the key of a graph without a kept atom, mix(0).  The kernel and the tests' restatement
# share these names and nothing else.
KEY_MIX_GAMMA, KEY_MIX_M1, KEY_MIX_M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
KEY_MIX_SHIFTS = (30, 27, 31)
KEY_ROUNDS = 3
KEY_NO_PATH = 255
KEY_EMPTY = 0xE220A8397B1DCDAF
_M64 = (1 << 64) - 1

# The fingerprint (DESIGN.md 2.9 "Fingerprints and similarity"): bits and 64-bit words of a row (bit b is bit b & 63 of word b >> 6),
# the largest and the default radius.  The kernel and the tests' restatement share these names and nothing else.
FP_BITS = 2048
FP_WORDS = FP_BITS // 64
FP_MAX_RADIUS = 4
FP_RADIUS = 2

# The geometry screen (DESIGN.md 2.9 "Geometry"): status bits, and the names of the metric and count columns in the kernel's order
GEOM_BOND_SHORT = 1              # a bond shorter than bond_min
GEOM_BOND_LONG = 2               # a bond longer than bond_max
GEOM_CLASH = 4                   # two kept atoms without a bond closer than clash_min
GEOM_EX_CLASH = 8                # a kept atom closer than ex_clear to an exclusion sphere's centre
GEOM_FEATURE_MISSED = 16         # informational: a feature point without a kept atom closer than feat_cut
GEOM_NONFINITE = 32              # a kept-class atom or a point with a non-finite coordinate
GEOM_FAIL_MASK = GEOM_BOND_SHORT | GEOM_BOND_LONG | GEOM_CLASH | GEOM_EX_CLASH | GEOM_NONFINITE
GEOM_NAMES = {GEOM_BOND_SHORT: 'BOND_SHORT', GEOM_BOND_LONG: 'BOND_LONG', GEOM_CLASH: 'CLASH', GEOM_EX_CLASH: 'EX_CLASH',
              GEOM_FEATURE_MISSED: 'FEATURE_MISSED', GEOM_NONFINITE: 'NONFINITE'}
GEOM_METRICS = ('bond_min', 'bond_max', 'nonbonded_min', 'ex_min', 'feature_max', 'centre_dist', 'bond_energy', 'reserved')
GEOM_COUNTS = ('bonds_short', 'bonds_long', 'clashes', 'ex_clashes', 'features_covered', 'features')

# The ring screen (DESIGN.md 2.9 "Rings"): status bits, and the names of the count columns in the kernel's order
RING_AROMATIC_OUTSIDE = 1        # a bond of order 4 that is in no ring
RING_SMALL = 2                   # a ring bond whose smallest ring has fewer than ring_min atoms
RING_LARGE = 4                   # a ring bond whose smallest ring has more than ring_max atoms
RING_SYSTEM_LARGE = 8            # a ring system of more than system_max atoms
RING_ROTATABLE = 16              # more than rotatable_max rotatable bonds
RING_AROMATIC_LONE = 32          # informational: an atom with exactly one bond of order 4
RING_FAIL_MASK = RING_AROMATIC_OUTSIDE | RING_SMALL | RING_LARGE | RING_SYSTEM_LARGE | RING_ROTATABLE
RING_NAMES = {RING_AROMATIC_OUTSIDE: 'AROMATIC_OUTSIDE', RING_SMALL: 'SMALL', RING_LARGE: 'LARGE', RING_SYSTEM_LARGE: 'SYSTEM_LARGE',
              RING_ROTATABLE: 'ROTATABLE', RING_AROMATIC_LONE: 'AROMATIC_LONE'}
RING_COUNTS = ('rings', 'ring_bonds', 'ring_atoms', 'ring_systems', 'ring_min', 'ring_max', 'largest_system', 'rotatable',
               'aromatic_outside_ring', 'aromatic_lone')

# The Kekulé form (DESIGN.md 2.9 "Kekulé form"): status bits, the names of the count columns in the kernel's order, and the tables
# the kernel is handed, per element in ATOM_TYPES order.  With s = the sum of an atom's non-aromatic bond orders and a = its aromatic
# bonds, an aromatic atom may carry the ring double bond in neutral form iff s + a + 1 <= KEKULE_DBL_NEUTRAL, as a cation iff
# s + a + 1 <= KEKULE_DBL_CHARGED; an atom with KEKULE_MUST that can carry one must get one.  H_VALENCES: the valences hydrogens fill
# an atom up to (the smallest that is not below what it already has).
# CAVEAT, as for MAX_VALENCE: written from memory; RDKit is not a dependency of this project and the tables have not been checked
# against it.  These are the tables' only copies: the kernel and the tests' restatement are handed them.
KEKULE_FAILED = 1                # neither the neutral nor (if allowed) the charged pass has a Kekulé structure
KEKULE_CHARGED = 2               # informational: the structure is the charged pass's (never together with KEKULE_FAILED)
KEKULE_HAS_AROMATIC = 4          # informational: an atom with a bond of order 4
KEKULE_CATION = 8                # informational: an atom with a charge
KEKULE_FAIL_MASK = KEKULE_FAILED
KEKULE_NAMES = {KEKULE_FAILED: 'FAILED', KEKULE_CHARGED: 'CHARGED', KEKULE_HAS_AROMATIC: 'HAS_AROMATIC', KEKULE_CATION: 'CATION'}
KEKULE_COUNTS = ('aromatic_atoms', 'aromatic_bonds', 'doubled', 'must_atoms', 'may_matched', 'hydrogens', 'charge', 'hbd', 'hba',
                 'heavy_atoms')
_KEKULE_KEYS = {k: 'net_charge' if k == 'charge' else k for k in KEKULE_COUNTS}   # (a molecule's dict has 'charge' per atom)
KEKULE_DBL_NEUTRAL = {5: 0, 6: 4, 7: 3, 8: 0, 9: 0, 14: 4, 15: 3, 16: 0, 17: 0, 35: 0, 53: 0}
KEKULE_DBL_CHARGED = {5: 0, 6: 0, 7: 4, 8: 0, 9: 0, 14: 0, 15: 4, 16: 3, 17: 0, 35: 0, 53: 0}
KEKULE_MUST = {5: 0, 6: 1, 7: 0, 8: 0, 9: 0, 14: 1, 15: 0, 16: 0, 17: 0, 35: 0, 53: 0}
H_VALENCES = {5: (3,), 6: (4,), 7: (3,), 8: (2,), 9: (1,), 14: (4,), 15: (3, 5), 16: (2, 4, 6), 17: (1,), 35: (1,), 53: (1, 3, 5)}
assert list(KEKULE_DBL_NEUTRAL) == list(KEKULE_DBL_CHARGED) == list(KEKULE_MUST) == list(H_VALENCES) == ATOM_TYPES
# The feature typing (DESIGN.md 2.9 "Features"): the typed feature types in the order of the bits of an atom's byte, status bits, and
# the names of the count columns in the kernel's order
FEATURE_TYPES = ('HD', 'AR', 'PO', 'HA', 'HY', 'NE', 'XB')
FEAT_NO_KEKULE = 1               # the graph has no Kekulé structure: nothing to type from, every typed point is unmatched
FEAT_UNMATCHED = 2               # more than max_unmatched typed points without an atom of their type closer than feat_cut
FEAT_HAS_UNTYPED = 4             # informational: a feature point of a type that is not typed (MB, CV1..CV4, CR)
FEAT_NONFINITE = 8               # a kept atom or a feature point with a non-finite coordinate
FEAT_FAIL_MASK = FEAT_NO_KEKULE | FEAT_UNMATCHED | FEAT_NONFINITE
FEAT_NAMES = {FEAT_NO_KEKULE: 'NO_KEKULE', FEAT_UNMATCHED: 'UNMATCHED', FEAT_HAS_UNTYPED: 'HAS_UNTYPED', FEAT_NONFINITE: 'NONFINITE'}
FEATURE_COUNTS = (('typed_points', 'matched', 'unmatched', 'untyped_points') + tuple('atoms_' + t for t in FEATURE_TYPES)
                  + tuple('points_' + t for t in FEATURE_TYPES) + tuple('matched_' + t for t in FEATURE_TYPES))
POINT_UNTYPED, POINT_IGNORED = -1, -2   # point kinds beside 0..6: a feature that is not typed; an exclusion sphere
_TYPES_OF_BYTE = [tuple(t for k, t in enumerate(FEATURE_TYPES) if b >> k & 1) for b in range(256)]    # an `atom_fp` byte -> its type names

# The SMILES writer (DESIGN.md 2.9 "SMILES"): status bits, the names of the count columns in the kernel's order, and the notation's
# own table: the OpenSMILES normal valences of the elements that may be written without brackets, per element in ATOM_TYPES order (an
# empty list: the element is always bracketed).  A bare atom is read with (the smallest entry that is not below the sum of its bond
# orders) - (that sum) hydrogens, 0 without such an entry.  This is a second table next to H_VALENCES on purpose: it belongs to the
# notation, not to the hydrogen rule; where the two disagree (N above 3, I above 1) the atom is written in brackets.  This is the
# table's only copy: the kernel and the tests' restatement are handed it.
SMILES_NO_KEKULE = 1             # the graph's Kekulé status has KEKULE_FAILED: nothing to write from
SMILES_RING_LABELS = 2           # more than 99 ring-closure labels would be in use at once
SMILES_TOO_LONG = 4              # the text needs more bytes than the row's capacity (the count 'length' says how many)
SMILES_DISCONNECTED = 8          # informational: the text has a '.'
SMILES_EMPTY = 16                # informational: no kept atom, the text is empty (the screen says NO_ATOMS)
SMILES_BRACKET = 32              # informational: at least one bracket atom
SMILES_FAIL_MASK = SMILES_NO_KEKULE | SMILES_RING_LABELS | SMILES_TOO_LONG
SMILES_NAMES = {SMILES_NO_KEKULE: 'NO_KEKULE', SMILES_RING_LABELS: 'RING_LABELS', SMILES_TOO_LONG: 'TOO_LONG',
                SMILES_DISCONNECTED: 'DISCONNECTED', SMILES_EMPTY: 'EMPTY', SMILES_BRACKET: 'BRACKET'}
SMILES_COUNTS = ('length', 'atoms', 'bonds', 'components', 'ring_closures', 'branches', 'max_label', 'bracket_atoms')
SMILES_VALENCES = {5: (3,), 6: (4,), 7: (3, 5), 8: (2,), 9: (1,), 14: (), 15: (3, 5), 16: (2, 4, 6), 17: (1,), 35: (1,), 53: (1,)}
SMILES_MAX_LABEL = 99
# pg_mol_smiles_stereo only (kept out of SMILES_NAMES / SMILES_COUNTS, which describe pg_mol_smiles)
SMILES_STEREO_DROPPED = 64       # informational: the marks of a group of double bonds contradicted each other and were left out
SMILES_STEREO_COUNTS = ('centres', 'centres_clockwise', 'marked_bonds', 'double_bonds')
assert list(SMILES_VALENCES) == ATOM_TYPES

# The stereo perception (DESIGN.md 2.9 "Stereo"): status bits, the names of the count columns in the kernel's order, the value of an
# element that is stereogenic but whose geometry does not decide, and the four words of the stereo key
STEREO_NO_KEKULE = 1             # the graph's Kekulé status has KEKULE_FAILED: nothing to perceive from
STEREO_UNDEFINED = 2             # more than max_undefined stereogenic elements whose geometry does not decide
STEREO_HAS_CENTRE = 4            # informational: at least one centre with parity +1 or -1
STEREO_HAS_BOND = 8              # informational: at least one double bond that is cis or trans
STEREO_NONFINITE = 16            # a kept atom with a non-finite coordinate
STEREO_FAIL_MASK = STEREO_NO_KEKULE | STEREO_UNDEFINED | STEREO_NONFINITE
STEREO_NAMES = {STEREO_NO_KEKULE: 'NO_KEKULE', STEREO_UNDEFINED: 'UNDEFINED', STEREO_HAS_CENTRE: 'HAS_CENTRE', STEREO_HAS_BOND: 'HAS_BOND',
                STEREO_NONFINITE: 'NONFINITE'}
STEREO_COUNTS = ('centre_candidates', 'centres_stereogenic', 'centres_defined', 'centres_undefined', 'bond_candidates',
                 'bonds_stereogenic', 'bonds_defined', 'bonds_undefined')
STEREO_UNDEFINED_VALUE = 2
STEREO_CENTRE_CLASSES = (6, 7, 14, 15, 16)       # atomic numbers of the elements that can be centres
STEREO_KEY_A, STEREO_KEY_B = 0x243F6A8885A308D3, 0x13198A2E03707344      # a centre with label +1 / -1
STEREO_KEY_C, STEREO_KEY_D = 0xA4093822299F31D0, 0x082EFA98EC4E6C89      # a double bond with label +1 / -1

# Standard atomic weights for 'mol_weight' (written from memory, abridged values)
ATOMIC_WEIGHT = {1: 1.008, 5: 10.81, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998, 14: 28.085, 15: 30.974, 16: 32.06, 17: 35.45,
                 35: 79.904, 53: 126.904}


_BOUND_TEXT = {0x7fffffff: '2**31 - 1', 1 << 30: '2**30'}


def _check_int(fn, name, v, lo, hi):
    """v as an int if it is an integer (no bool) in lo .. hi, else the ValueError of `fn`."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f'{fn}: {name} must be an integer in {lo} .. {_BOUND_TEXT.get(hi, hi)}, not {v!r}')
    return int(v)


def _check_number(fn, name, v, positive):
    """A finite number (no bool) >= 0, or > 0 with `positive`, else the ValueError of `fn`."""
    if (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0
            or (positive and v == 0)):
        raise ValueError(f'{fn}: {name} must be a finite number {">" if positive else ">="} 0, not {v!r}')


@dataclass(frozen=True)
class KekuleOptions:
    """allow_charged: if the neutral pass has no Kekulé structure, try again with N+ / P+ / S+ carrying a ring double bond."""
    allow_charged: bool = True

    def __post_init__(self):
        if not isinstance(self.allow_charged, (bool, np.bool_)):
            raise ValueError(f'KekuleOptions: allow_charged must be a bool, not {self.allow_charged!r}')


@dataclass(frozen=True)
class RingLimits:
    """Limits of the ring screen, in atoms / bonds.  The defaults cannot be broken by a graph of MAX_ATOMS atoms (no ring below 3 or
    above 128 atoms, no system above 128, at most 8128 bonds), so with them only the aromatic rule can fail; the others are the user's
    filters, e.g. RingLimits(ring_min=5, ring_max=8).  RING_SMALL: 0 < smallest ring < ring_min; the other three: value > limit."""
    ring_min: int = 3
    ring_max: int = 128
    system_max: int = 128
    rotatable_max: int = 8128

    def __post_init__(self):
        for k, v in zip(('ring_min', 'ring_max', 'system_max', 'rotatable_max'), astuple(self)):
            _check_int('RingLimits', k, v, 0, 0x7fffffff)


@dataclass(frozen=True)
class FeatureLimits:
    """Limits of the typed feature match.  feat_cut: `check_nearby_phore`'s cutoff in Angstrom (utils/phore_utils.py:406), the
    comparison is strict; max_unmatched: FEAT_UNMATCHED is set when more typed points than this have no atom of their type within
    feat_cut.  With the defaults only FEAT_NO_KEKULE / FEAT_NONFINITE can fail; FeatureLimits(max_unmatched=0) asks for every typed
    feature."""
    feat_cut: float = 2.0
    max_unmatched: int = 2 ** 31 - 1

    def __post_init__(self):
        _check_number('FeatureLimits', 'feat_cut', self.feat_cut, False)
        _check_int('FeatureLimits', 'max_unmatched', self.max_unmatched, 0, 0x7fffffff)


@dataclass(frozen=True)
class GeomLimits:
    """Limits of the geometry screen in Angstrom; every comparison is strict.  bond_min / bond_max: `compute_atom_prox_loss`'s min_d /
    max_d (utils/sample_utils.py:135); ex_clear: the clearance `exclude_clashed_ex(low=3.0)` keeps between exclusion spheres and ligand
    atoms (utils/phore_utils.py:511); feat_cut: `check_nearby_phore`'s cutoff (utils/phore_utils.py:406).  clash_min has no value in the
    reference: it is bond_min, as a one-sided rule -- atoms without a bond closer than the shortest tolerated bond are wrong."""
    bond_min: float = 1.2
    bond_max: float = 2.8
    clash_min: float = 1.2
    ex_clear: float = 3.0
    feat_cut: float = 2.0


@dataclass(frozen=True)
class StereoLimits:
    """Thresholds of the stereo perception.  vol_min: a centre is defined iff |V| >= vol_min, V the signed volume of its four unit
    ligand vectors (an ideal tetrahedron has |V| = 3.08, a planar atom 0); planar_min: a double bond is cis / trans iff |t| >=
    planar_min, t the normalised product of its two substituents' components across the bond (ideal sp2: 0.75, perpendicular: 0);
    max_undefined: STEREO_UNDEFINED is set when more stereogenic elements than this are undefined.  The two thresholds are design
    choices, about a sixth and a third of the ideal values; they are NOT calibrated on sampled molecules.  This is their only copy:
    the kernel and the tests' restatement are handed them."""
    vol_min: float = 0.5
    planar_min: float = 0.25
    max_undefined: int = 2 ** 31 - 1

    def __post_init__(self):
        for k in ('vol_min', 'planar_min'):
            _check_number('StereoLimits', k, getattr(self, k), True)
        _check_int('StereoLimits', 'max_undefined', self.max_undefined, 0, 0x7fffffff)


@dataclass(frozen=True)
class BondMargins:
    """Margins of the distance bond rule in pm (the reference's margin1 / margin2 / margin3): a pair is bonded iff 100 d < single +
    `single`, then double iff 100 d < double + `double`, then triple iff 100 d < triple + `triple`; every comparison is strict and in
    fp32.  A pair without a table entry never takes that order, whatever the margin."""
    single: float = 10
    double: float = 5
    triple: float = 3

    def __post_init__(self):
        for k in ('single', 'double', 'triple'):
            _check_number('BondMargins', k, getattr(self, k), False)


def _pad4(table):
    return [list(table[z]) + [0] * (4 - len(table[z])) for z in ATOM_TYPES]


# The tables the kernels are handed, as rows of uint8 in class order: twice MAX_VALENCE [11]; KEKULE_DBL_NEUTRAL, KEKULE_DBL_CHARGED,
# KEKULE_MUST [11] and H_VALENCES [11, 4]; SMILES_VALENCES [11, 4]
_TABLE_ROWS = {'valence': ([2 * MAX_VALENCE[z] for z in ATOM_TYPES],),
               'kekule': tuple([d[z] for z in ATOM_TYPES] for d in (KEKULE_DBL_NEUTRAL, KEKULE_DBL_CHARGED, KEKULE_MUST)) + (_pad4(H_VALENCES),),
               'smiles': (_pad4(SMILES_VALENCES),)}


@lru_cache(maxsize=None)
def _tables(name, device):
    """The tensors of _TABLE_ROWS[name] on `device`, made once per device."""
    return tuple(torch.tensor(r, dtype=torch.uint8, device=device) for r in _TABLE_ROWS[name])


def bond_thresholds(margins=None):
    """The distance rule's thresholds as the kernel takes them: fp32 [11, 11, 3] in ATOM_TYPES order, `length + margin` in pm, 0 where
    the table has no entry (no distance is below 0, so such a pair never takes that order)."""
    margins = BondMargins() if margins is None else margins
    length = np.asarray(BOND_LENGTHS_PM, dtype=np.float64).transpose(1, 2, 0)
    return np.ascontiguousarray(np.where(length > 0, length + np.asarray(astuple(margins), dtype=np.float64), 0.0), dtype=np.float32)


@lru_cache(maxsize=None)
def _bond_threshold_table(margins, device):
    """`bond_thresholds(margins)` on `device`, made once per margins and device."""
    return torch.from_numpy(bond_thresholds(margins)).to(device)


def _valence_table(device):
    return _tables('valence', device)[0]


def _kekule_table(device):
    return _tables('kekule', device)


def _smiles_table(device):
    return _tables('smiles', device)[0]


@dataclass
class Screen:
    """Device tensors of one `screen` call; F frames, B graphs, N atom rows, E directed bond rows (H = E / 2 pairs a < b)."""
    status: torch.Tensor         # int32 [F, B]   STATUS_* bits
    counts: torch.Tensor         # int32 [F, B, 4] kept atoms, bonds, components, atoms of the largest component
    valid: torch.Tensor          # bool  [F, B]   no bit of FAIL_MASK
    cls: torch.Tensor            # int8  [F, N]   atom class, -1 = dropped
    compact: torch.Tensor        # int16 [F, N]   index among the kept atoms of the graph, -1 = dropped
    valence2: torch.Tensor       # uint8 [F, N]   twice the valence (aromatic = 1.5), saturating at 255
    comp: torch.Tensor           # int16 [F, N]   smallest local atom index of the atom's component, -1 = dropped
    order: torch.Tensor          # int8  [F, H]   bond order of the pair rows (0 = none, 4 = aromatic); graph g starts at bond_off[g] / 2
    lig_off: torch.Tensor        # int32 [B + 1]
    bond_off: torch.Tensor       # int32 [B + 1]  (directed rows, both halves)
    num_atoms: list              # B ints
    bonds: str = 'predicted'     # where `order` comes from: 'predicted' (argmax of the edge scores) or 'distance' (the coordinates)
    agree: torch.Tensor = None   # int32 [F, B, 6] BOND_AGREE_COUNTS; `bond_agreement` only


def _need_cuda(fn, noun, dev, holder='result'):
    if dev.type != 'cuda':
        raise RuntimeError(f'phoregen_amd.molecule.{fn}: {noun} is a HIP kernel and the {holder} lives on {dev}; there is no CPU fallback')


def _check_rows(fn, t, F, k, what, dev):
    """t is [rows, k] or [F, rows, k]: fp32 on dev, every frame contiguous (the frames may be strided)."""
    row = t[0] if t.dim() == 3 and F > 0 else t
    if t.dtype != torch.float32 or t.device != dev or t.size(-1) != k or not (row.is_contiguous() or row.numel() == 0):
        raise ValueError(f'phoregen_amd.molecule.{fn}: {what} must be contiguous fp32 [.., {k}] on one device')


def _check_arrays(who, dev, arrays):
    """arrays: (tensor, dtype) pairs in the order of the launch; each must be contiguous, of that dtype and on dev."""
    for i, (t, dt) in enumerate(arrays):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f'phoregen_amd.molecule.{who}: array {i} of the launch must be contiguous {dt} on {dev}, it is '
                             f'{"" if t.is_contiguous() else "non-contiguous "}{t.dtype} on {t.device}')


def _screen_of(fn, screen, results, frames, F, N, E, dev):
    """The `Screen` a function works on: the one handed in, else a new one; it must be one of this result and frames."""
    sc = screen if screen is not None else _screen(results, frames)
    if tuple(sc.status.shape) != (F, len(sc.num_atoms)) or sc.cls.size(1) != N or sc.cls.device != dev or 2 * sc.order.size(1) != E:
        raise ValueError(f'phoregen_amd.molecule.{fn}: the screen ({tuple(sc.status.shape)} frames x graphs, {sc.cls.size(1)} atom '
                         f'rows) is not one of this result and frames ({F} frames, {N} atom rows)')
    return sc


def _same_screen(a, b):
    return a is b or not (a.num_atoms != b.num_atoms or a.status.shape != b.status.shape or a.cls.shape != b.cls.shape
                          or a.order.shape != b.order.shape or a.cls.device != b.cls.device or a.bonds != b.bonds)


def _resolve(fn, results, frames, screen, where='phoregen_amd.molecule', **given):
    """The one `Screen` a function and the results it was handed (name=result, None: not handed in) work on: screen= if given, else
    the first result's, else a new one.  It must be one of this result and frames, and every result must have been computed from
    it.  A `MolKeys` (keys=) carries no screen: its shapes are held against it."""
    node, _, edge, F, _ = _frames(results, frames)
    given = {what: x for what, x in given.items() if x is not None}
    first = next((x.screen for what, x in given.items() if what != 'keys'), None)
    sc = _screen_of(fn, screen if screen is not None else first, results, frames, F, node.size(-2), edge.size(-2), node.device)
    for what, x in given.items():
        if (what == 'keys' and (x.key.shape != sc.status.shape or x.colour.shape != sc.cls.shape or x.key.device != sc.cls.device)
                or what != 'keys' and not _same_screen(sc, x.screen)):
            raise ValueError(f'{where}.{fn}: screen= and {what}= were computed from screens of different results')
    return sc


def _point_count(fn, point_pos):
    if not torch.is_tensor(point_pos) or point_pos.dim() != 2 or point_pos.size(1) != 3:
        raise ValueError(f'phoregen_amd.molecule.{fn}: point_pos must be a tensor [P, 3]')
    return point_pos.size(0)


def _frames(results, frames):
    if frames == 'final':
        node, pos, edge = results['pred']
        return node, pos, edge, 1, (0, 0, 0)
    if frames == 'traj':
        node, pos, edge = results['traj']
        if node is None or pos is None or edge is None:
            raise ValueError("phoregen_amd.molecule.screen: frames='traj' needs a result sampled with return_traj=True")
        if not (node.dim() == pos.dim() == edge.dim() == 3 and node.size(0) == pos.size(0) == edge.size(0)):
            raise ValueError('phoregen_amd.molecule.screen: trajectory tensors must be [frames, rows, .] with one frame count')
        return node, pos, edge, node.size(0), (node.stride(0), edge.stride(0), pos.stride(0))
    raise ValueError(f"phoregen_amd.molecule.screen: frames must be 'final' or 'traj', not {frames!r}")


@torch.no_grad()
def screen(results, frames='final', bonds='predicted', margins=BondMargins()):
    """Decode and screen every graph of a `sample` / `sample_batch` result on the device its tensors live on.
    frames='final': the final prediction (`results['pred']`, F = 1); 'traj': every frame of the saved trajectory.
    bonds='predicted': the order of a pair is the argmax of its edge scores (pg_mol_screen).  bonds='distance': it is perceived from
    the coordinates with the reference's `--add_edge distance` rule (pg_mol_screen_dist; BOND_LENGTHS_PM, `margins`; DESIGN.md 2.9
    "Distance bonds"): orders 1..3 only, the edge scores are not read, the status may carry STATUS_DIST_UNMAPPED_ELEMENT and never
    STATUS_HAD_ABSORBING_BOND.  The `Screen` has the same arrays either way, so everything that takes one works on either.
    `results` is only read."""
    return _screen_any(results, frames, bonds, margins, False)


def _screen_any(results, frames, bonds, margins, _agree):
    """`screen`; _agree: with bonds='distance', also read the edge scores and fill `Screen.agree`."""
    if bonds not in BOND_MODES:
        raise ValueError(f'phoregen_amd.molecule.screen: bonds must be one of {BOND_MODES}, not {bonds!r}')
    if not isinstance(margins, BondMargins):
        raise ValueError(f'phoregen_amd.molecule.screen: margins must be a BondMargins, not {margins!r}')
    node, pos, edge, F, (node_fs, edge_fs, pos_fs) = _frames(results, frames)
    dev = node.device
    _need_cuda('screen', 'the screen', dev)
    for t, k, what in ((node, 12, 'atom scores'), (pos, 3, 'coordinates'), (edge, 6, 'bond scores')):
        _check_rows('screen', t, F, k, what, dev)
    N, E = node.size(-2), edge.size(-2)
    na = results['lig_info'][0].to(dev).long().reshape(-1)
    B = na.numel()
    with torch.cuda.device(dev):
        lib = hip.lib()
        lig_off = torch.zeros(B + 1, dtype=torch.long, device=dev)
        bond_off = torch.zeros(B + 1, dtype=torch.long, device=dev)
        lig_off[1:], bond_off[1:] = na.cumsum(0), (na * (na - 1)).cumsum(0)
        num_atoms = na.tolist()                                        # (the one host read of this call)
        if any(n < 0 for n in num_atoms) or sum(num_atoms) != N or pos.size(-2) != N:
            raise ValueError(f'phoregen_amd.molecule.screen: num_atoms sum to {sum(num_atoms)}, the result has {N} atom rows')
        if sum(n * (n - 1) for n in num_atoms) != E:
            raise ValueError(f'phoregen_amd.molecule.screen: {E} bond rows, num_atoms imply {sum(n * (n - 1) for n in num_atoms)} '
                             '(fully connected, both directions)')
        lig_off, bond_off = lig_off.int(), bond_off.int()
        H = E // 2
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev), counts=torch.empty(F, B, 4, dtype=torch.int32, device=dev),
                   cls=torch.empty(F, N, dtype=torch.int8, device=dev), compact=torch.empty(F, N, dtype=torch.int16, device=dev),
                   valence2=torch.empty(F, N, dtype=torch.uint8, device=dev), comp=torch.empty(F, N, dtype=torch.int16, device=dev),
                   order=torch.empty(F, H, dtype=torch.int8, device=dev))
        agree = None
        if bonds == 'predicted':
            _launch(lib, node, node_fs, edge, edge_fs, pos, pos_fs, lig_off, bond_off, B, F, N, E, max(num_atoms, default=0), out)
        else:
            agree = torch.empty(F, B, len(BOND_AGREE_COUNTS), dtype=torch.int32, device=dev) if _agree else None
            _launch_dist(lib, node, node_fs, pos, pos_fs, edge if _agree else None, edge_fs, lig_off, bond_off, B, F, N, E,
                         max(num_atoms, default=0), _bond_threshold_table(margins, dev), out, agree)
    return Screen(valid=(out['status'] & FAIL_MASK) == 0, lig_off=lig_off, bond_off=bond_off, num_atoms=num_atoms, bonds=bonds,
                  agree=agree, **out)


def bond_agreement(results, frames='final', margins=BondMargins()):
    """The distance `Screen` of `screen(bonds='distance')` with `agree` filled: int32 [F, B, 6], per (frame, graph) the pairs a < b of
    kept atoms with finite coordinates counted by how the predicted bond (argmax of the pair's edge scores; class 5 is no bond) and
    the distance bond agree (BOND_AGREE_COUNTS).  One launch; the reversed half of the edge rows is not read."""
    return _screen_any(results, frames, 'distance', margins, True)


_screen = screen                 # (functions below take a `screen=` argument)


@dataclass
class MolKeys:
    """Device tensors of one `molecule_keys` call.  The int64 values are 64-bit patterns: read them as unsigned (`& 2**64 - 1`)."""
    key: torch.Tensor            # int64 [F, B]   identity key of the decoded molecule (KEY_EMPTY where no atom was kept)
    colour: torch.Tensor         # int64 [F, N]   final refinement colour of a kept atom, 0 = dropped


@torch.no_grad()
def molecule_keys(sc):
    """Identity keys of every (frame, graph) of a `Screen`, on its device, in one launch (pg_mol_key).  The key depends on the kept
    atoms' elements and the bonds' orders alone (4 = aromatic is its own label), not on the numbering of the atoms, coordinates,
    dropped atoms or absorbing rows.  Equal keys are NECESSARY, not sufficient, for equal molecules: `same_molecule` decides."""
    dev = sc.cls.device
    _need_cuda('molecule_keys', 'the key', dev, 'screen')
    F, B = sc.status.shape
    with torch.cuda.device(dev):
        lib = hip.lib()
        key = torch.empty(F, B, dtype=torch.int64, device=dev)
        colour = torch.empty(F, sc.cls.size(1), dtype=torch.int64, device=dev)
        _launch_key(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms, default=0), key, colour)
    return MolKeys(key=key, colour=colour)


def _launch_key(lib, cls, order, lig_off, bond_off, B, F, max_n, key, colour):
    """pg_mol_key on the current stream; `colour` may be None.  A graph above MAX_ATOMS is the library's error: nothing is launched
    and the outputs are not written."""
    _check_arrays('molecule_keys', cls.device, [(cls, torch.int8), (order, torch.int8), (lig_off, torch.int32), (bond_off, torch.int32)])
    hip.check(lib.pg_mol_key(cls.data_ptr(), order.data_ptr(), lig_off.data_ptr(), bond_off.data_ptr(), B, F, cls.size(-1),
                             2 * order.size(-1), max_n, key.data_ptr(), hip.ptr(colour), hip.stream_ptr()), 'pg_mol_key')


@dataclass
class Fingerprints:
    """Device tensors of one `fingerprints` call.  The int64 values are 64-bit patterns: read them as unsigned (`& 2**64 - 1`)."""
    fp: torch.Tensor             # int64 [F, B, 32] bit b of a row is bit b & 63 of word b >> 6
    bits: torch.Tensor           # int32 [F, B]     set bits of the row
    radius: int
    screen: Screen = None        # the screen it was computed from


def _check_radius(fn, radius):
    return _check_int(f'phoregen_amd.molecule.{fn}', 'radius', radius, 0, FP_MAX_RADIUS)


@torch.no_grad()
def fingerprints(sc, radius=FP_RADIUS):
    """Circular fingerprints of every (frame, graph) of a `Screen`, on its device, in one launch (pg_mol_fp; DESIGN.md 2.9
    "Fingerprints and similarity"): FP_BITS bits per molecule, one for every kept atom's environment identifier of radius 0 .. radius
    (the identity key's initial colour, then `radius` rounds over the atom's bonds).  It depends on the kept atoms' elements and the
    bonds' orders alone (4 = aromatic is its own order: no kekulisation, so it does not depend on which Kekulé structure `kekulize`
    returns), not on the numbering of the atoms, coordinates, dropped atoms or absorbing rows.  An empty graph has no bit set; a
    disconnected one has one fingerprint.  `phoregen_amd.similarity` compares them.  This is NOT RDKit's ECFP: no duplicate-
    environment removal, other atom invariants, another hash; not checked against RDKit."""
    radius = _check_radius('fingerprints', radius)
    dev = sc.cls.device
    _need_cuda('fingerprints', 'the fingerprint', dev, 'screen')
    F, B = sc.status.shape
    with torch.cuda.device(dev):
        lib = hip.lib()
        fp = torch.empty(F, B, FP_WORDS, dtype=torch.int64, device=dev)
        bits = torch.empty(F, B, dtype=torch.int32, device=dev)
        _launch_fp(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms, default=0), radius, fp, bits)
    return Fingerprints(fp=fp, bits=bits, radius=radius, screen=sc)


def _launch_fp(lib, cls, order, lig_off, bond_off, B, F, max_n, radius, fp, bits):
    """pg_mol_fp on the current stream.  A graph above MAX_ATOMS or a radius outside 0 .. FP_MAX_RADIUS is the library's error:
    nothing is launched and the outputs are not written."""
    _check_arrays('fingerprints', cls.device, [(cls, torch.int8), (order, torch.int8), (lig_off, torch.int32), (bond_off, torch.int32),
                                               (fp, torch.int64), (bits, torch.int32)])
    if (lig_off.numel() != B + 1 or bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or fp.numel() != F * B * FP_WORDS or bits.numel() != F * B):
        raise ValueError(f'phoregen_amd.molecule.fingerprints: sizes of the offsets, screen arrays and outputs do not fit {F} frames x '
                         f'{B} graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_fp(cls.data_ptr(), order.data_ptr(), lig_off.data_ptr(), bond_off.data_ptr(), B, F, cls.size(-1),
                            2 * order.size(-1), max_n, radius, fp.data_ptr(), bits.data_ptr(), hip.stream_ptr()), 'pg_mol_fp')


def _launch(lib, node, node_fs, edge, edge_fs, pos, pos_fs, lig_off, bond_off, B, F, N, E, max_n, out):
    """pg_mol_screen on the current stream.  A graph above MAX_ATOMS is the library's error (RuntimeError with its message): nothing
    is launched and `out` is not written."""
    hip.check(lib.pg_mol_screen(node.data_ptr(), node_fs, edge.data_ptr(), edge_fs, pos.data_ptr(), pos_fs, lig_off.data_ptr(),
                                bond_off.data_ptr(), B, F, N, E, max_n, _valence_table(node.device).data_ptr(),
                                out['status'].data_ptr(), out['counts'].data_ptr(), out['cls'].data_ptr(),
                                out['compact'].data_ptr(), out['valence2'].data_ptr(), out['comp'].data_ptr(),
                                out['order'].data_ptr(), hip.stream_ptr()), 'pg_mol_screen')


def _launch_dist(lib, node, node_fs, pos, pos_fs, edge, edge_fs, lig_off, bond_off, B, F, N, E, max_n, thresholds, out, agree):
    """pg_mol_screen_dist on the current stream; edge / agree: None, or the edge scores and the [F, B, 6] output of the agreement
    counts.  A graph above MAX_ATOMS is the library's error (RuntimeError with its message): nothing is launched and `out` is not
    written."""
    _check_arrays('screen', node.device, [(thresholds, torch.float32)] + ([] if agree is None else [(agree, torch.int32)]))
    if thresholds.numel() != 3 * len(ATOM_TYPES) ** 2 or (agree is not None and agree.numel() != F * B * len(BOND_AGREE_COUNTS)):
        raise ValueError('phoregen_amd.molecule.screen: the threshold table must be [11, 11, 3], the agreement counts [F, B, 6]')
    hip.check(lib.pg_mol_screen_dist(node.data_ptr(), node_fs, pos.data_ptr(), pos_fs, hip.ptr(edge), edge_fs, lig_off.data_ptr(),
                                     bond_off.data_ptr(), B, F, N, E, max_n, _valence_table(node.device).data_ptr(),
                                     thresholds.data_ptr(), out['status'].data_ptr(), out['counts'].data_ptr(), out['cls'].data_ptr(),
                                     out['compact'].data_ptr(), out['valence2'].data_ptr(), out['comp'].data_ptr(),
                                     out['order'].data_ptr(), hip.ptr(agree), hip.stream_ptr()), 'pg_mol_screen_dist')


@dataclass
class Geometry:
    """Device tensors of one `geometry` call; F frames, B graphs, Q = the graphs' point counts summed (graph g owns the columns
    point_off[g] .. point_off[g + 1] of the per-point tensors)."""
    status: torch.Tensor         # int32 [F, B]    GEOM_* bits
    metrics: torch.Tensor        # fp32  [F, B, 8] GEOM_METRICS
    counts: torch.Tensor         # int32 [F, B, 6] GEOM_COUNTS
    ok: torch.Tensor             # bool  [F, B]    no bit of GEOM_FAIL_MASK
    point_dist: torch.Tensor     # fp32  [F, Q]    distance of a point to the nearest kept atom (+inf: none)
    point_atom: torch.Tensor     # int16 [F, Q]    that atom's compact index (the screen's), -1: none
    point_off: torch.Tensor      # int32 [B + 1]
    point_range: torch.Tensor    # int32 [B, 2]    rows of the graph's points in the point tensors that were handed in
    limits: GeomLimits
    screen: Screen               # the screen it was measured on


def _point_ranges(point_batch, P, B, dev):
    """(ranges [B, 2], offsets [B + 1]) of the graphs' points, int32 on the device, without a host read of device data."""
    if point_batch is None:                                            # every graph has all points
        ranges = torch.tensor([0, P], dtype=torch.int32).repeat(B, 1)
        return ranges.to(dev), (torch.arange(B + 1, dtype=torch.int64) * P).int().to(dev)
    pb = point_batch.reshape(-1)
    if pb.numel() != P or pb.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'phoregen_amd.molecule.geometry: point_batch must hold one integer graph id per point ({P}), it has '
                         f'{pb.numel()} of {pb.dtype}')
    if pb.device.type == 'cpu' and P and (bool((pb[1:] < pb[:-1]).any()) or int(pb[0]) < 0 or int(pb[-1]) >= B):
        raise ValueError(f'phoregen_amd.molecule.geometry: point_batch must be sorted graph ids in 0 .. {B - 1}')
    # (a device tensor is taken as sorted: checking it would be a host read; the kernel skips a graph whose range does not fit)
    pb = pb.to(dev).long().contiguous()
    ids = torch.arange(B, device=dev)
    start, end = torch.searchsorted(pb, ids), torch.searchsorted(pb, ids, right=True)
    off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    off[1:] = (end - start).cumsum(0)
    return torch.stack([start, end], 1).int().contiguous(), off.int()


def _points(point_pos, point_batch, B, dev):
    """(ranges, offsets, Q = the point outputs of a frame, the points as contiguous fp32 on the device)"""
    P = point_pos.size(0)
    ranges, off = _point_ranges(point_batch, P, B, dev)
    return ranges, off, P * B if point_batch is None else P, point_pos.to(dev, torch.float32).contiguous()


@torch.no_grad()
def geometry(results, point_pos, point_is_ex, point_batch=None, frames='final', screen=None, limits=GeomLimits()):
    """Measure every decoded (frame, graph) of a `sample` / `sample_batch` result against its pharmacophore, on the device, in one
    launch (pg_mol_geom).  point_pos [P, 3]: the points in the coordinates the frames hold (world coordinates for the final
    prediction); point_is_ex [P]: non-zero = exclusion sphere, else feature.  point_batch=None: every graph has all P points (what
    `sample` draws); else sorted graph ids per point, as `sample_batch`'s batch_phore.  A `Screen` of the same result and frames is
    reused if handed in.  No host read beyond the screen's.  Necessary, not sufficient: a molecule that passes has plausible bond
    lengths and stays out of the spheres, nothing more; 'covered' says an atom is near a feature, not that it is the matching group."""
    _, pos, edge, F, (_, _, pos_fs) = _frames(results, frames)
    dev = pos.device
    _need_cuda('geometry', 'the geometry screen', dev)
    lim = tuple(float(v) for v in astuple(limits))
    if len(lim) != 5 or not all(np.isfinite(lim)):
        raise ValueError(f'phoregen_amd.molecule.geometry: limits must be five finite numbers, not {limits!r}')
    P = _point_count('geometry', point_pos)
    if not torch.is_tensor(point_is_ex) or point_is_ex.numel() != P:
        raise ValueError(f'phoregen_amd.molecule.geometry: {P} points, point_is_ex has {getattr(point_is_ex, "shape", None)}')
    sc = _screen_of('geometry', screen, results, frames, F, pos.size(-2), edge.size(-2), dev)
    B = len(sc.num_atoms)
    _check_rows('geometry', pos, F, 3, 'coordinates', dev)
    with torch.cuda.device(dev):
        lib = hip.lib()
        ranges, off, Q, ppos = _points(point_pos, point_batch, B, dev)
        pex = (point_is_ex.reshape(-1).to(dev) != 0).to(torch.uint8)
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev), metrics=torch.empty(F, B, 8, dtype=torch.float32, device=dev),
                   counts=torch.empty(F, B, 6, dtype=torch.int32, device=dev), point_dist=torch.empty(F, Q, dtype=torch.float32, device=dev),
                   point_atom=torch.empty(F, Q, dtype=torch.int16, device=dev))
        _launch_geom(lib, pos, pos_fs, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms, default=0), ppos, pex, ranges,
                     off, Q, lim, out)
    return Geometry(ok=(out['status'] & GEOM_FAIL_MASK) == 0, point_off=off, point_range=ranges, limits=limits, screen=sc, **out)


def geometry_for(data, results, frames='final', screen=None, limits=GeomLimits(), ex_col=12):
    """`geometry` with the pharmacophore of `data` as `PhoreDiff.sample` reads it: the points are data['phore'].pos + data.center
    (world coordinates, as the final prediction and the trajectory frames 1.. are), exclusion spheres are the rows with column
    `ex_col` of data['phore'].x equal to 1 (12 for zinc_300 / pdbbind, `PhoreDiff.ex_col`), every graph has all points.  Frames are
    measured in the coordinates they hold: trajectory frame 0 is stored without the centre, as in the reference, so its row says
    little unless data.center is zero."""
    ph = data['phore']
    return geometry(results, ph.pos.float() + data.center.to(ph.pos.device).float(), ph.x[:, ex_col] == 1, None, frames, screen, limits)


def _launch_geom(lib, pos, pos_fs, cls, order, lig_off, bond_off, B, F, max_n, point_pos, point_is_ex, ranges, off, n_out, limits, out):
    """pg_mol_geom on the current stream.  A graph above MAX_ATOMS is the library's error: nothing is launched and `out` is not
    written."""
    _check_arrays('geometry', pos.device, [(cls, torch.int8), (order, torch.int8), (lig_off, torch.int32), (bond_off, torch.int32),
                                           (point_pos, torch.float32), (point_is_ex, torch.uint8), (ranges, torch.int32), (off, torch.int32)])
    if (lig_off.numel() != B + 1 or bond_off.numel() != B + 1 or off.numel() != B + 1 or ranges.numel() != 2 * B or cls.numel() != F * cls.size(-1)
            or order.numel() != F * order.size(-1) or point_is_ex.numel() != point_pos.size(0) or pos.size(-2) != cls.size(-1)
            or tuple(out['point_dist'].shape) != (F, n_out) or tuple(out['point_atom'].shape) != (F, n_out)
            or out['status'].numel() != F * B or out['metrics'].numel() != 8 * F * B or out['counts'].numel() != 6 * F * B):
        raise ValueError('phoregen_amd.molecule.geometry: sizes of the offsets, ranges, screen arrays, points and outputs do not fit '
                         f'{F} frames x {B} graphs, {cls.size(-1)} atom rows, {point_pos.size(0)} points, {n_out} point outputs')
    hip.check(lib.pg_mol_geom(pos.data_ptr(), pos_fs, cls.data_ptr(), order.data_ptr(), lig_off.data_ptr(), bond_off.data_ptr(), B, F,
                              cls.size(-1), 2 * order.size(-1), max_n, point_pos.data_ptr(), point_is_ex.data_ptr(), point_pos.size(0),
                              ranges.data_ptr(), off.data_ptr(), n_out, (ctypes.c_float * 5)(*limits), out['point_dist'].data_ptr(),
                              out['point_atom'].data_ptr(), out['metrics'].data_ptr(), out['counts'].data_ptr(),
                              out['status'].data_ptr(), hip.stream_ptr()), 'pg_mol_geom')


@dataclass
class Rings:
    """Device tensors of one `rings` call; F frames, B graphs, N atom rows, H pair rows (as the screen's `order`)."""
    status: torch.Tensor         # int32 [F, B]     RING_* bits
    counts: torch.Tensor         # int32 [F, B, 10] RING_COUNTS
    ok: torch.Tensor             # bool  [F, B]     no bit of RING_FAIL_MASK
    ring_size: torch.Tensor      # uint8 [F, H]     atoms of the smallest ring through the bond of this pair row; 0 = bridge or no bond
    atom_ring: torch.Tensor      # uint8 [F, N]     atoms of the smallest ring through the atom; 0 = none (or dropped)
    ring_sys: torch.Tensor       # int16 [F, N]     smallest local atom index of the atom's ring system, -1 = none (or dropped)
    limits: RingLimits
    screen: Screen               # the screen it was computed from


@torch.no_grad()
def rings(results, frames='final', screen=None, limits=RingLimits()):
    """Ring perception of every decoded (frame, graph) of a `sample` / `sample_batch` result, on the device, in one launch
    (pg_mol_rings): per bond the smallest ring through it (0 = bridge), per atom the smallest ring through it and its ring system
    (rings that share an atom, spiro atoms included, are one system), ten counts (RING_COUNTS) and a status word (RING_* bits).
    A `Screen` of the same result and frames is reused if handed in.  No host read beyond the screen's.  `ok` is a separate answer
    from the screen's `valid`: with the default limits it fails only on an aromatic bond outside a ring.  No kekulisation, no ring
    list, no hydrogens; `rotatable` has no amide or terminal-group exceptions and is not RDKit's NumRotatableBonds."""
    node, _, edge, F, _ = _frames(results, frames)
    dev = node.device
    _need_cuda('rings', 'the ring screen', dev)
    if not isinstance(limits, RingLimits):
        raise ValueError(f'phoregen_amd.molecule.rings: limits must be a RingLimits, not {limits!r}')
    sc = _screen_of('rings', screen, results, frames, F, node.size(-2), edge.size(-2), dev)
    B, N = len(sc.num_atoms), node.size(-2)
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(RING_COUNTS), dtype=torch.int32, device=dev),
                   ring_size=torch.empty(F, sc.order.size(1), dtype=torch.uint8, device=dev),
                   atom_ring=torch.empty(F, N, dtype=torch.uint8, device=dev), ring_sys=torch.empty(F, N, dtype=torch.int16, device=dev))
        _launch_rings(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms, default=0), astuple(limits), out)
    return Rings(ok=(out['status'] & RING_FAIL_MASK) == 0, limits=limits, screen=sc, **out)


def _launch_rings(lib, cls, order, lig_off, bond_off, B, F, max_n, limits, out):
    """pg_mol_rings on the current stream.  A graph above MAX_ATOMS is the library's error: nothing is launched and `out` is not
    written."""
    _check_arrays('rings', cls.device, [(cls, torch.int8), (order, torch.int8), (lig_off, torch.int32), (bond_off, torch.int32),
                                        (out['ring_size'], torch.uint8), (out['atom_ring'], torch.uint8), (out['ring_sys'], torch.int16),
                                        (out['counts'], torch.int32), (out['status'], torch.int32)])
    if (lig_off.numel() != B + 1 or bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or out['ring_size'].shape != order.shape or out['atom_ring'].shape != cls.shape or out['ring_sys'].shape != cls.shape
            or out['status'].numel() != F * B or out['counts'].numel() != len(RING_COUNTS) * F * B):
        raise ValueError(f'phoregen_amd.molecule.rings: sizes of the offsets, screen arrays and outputs do not fit {F} frames x {B} graphs, '
                         f'{cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_rings(cls.data_ptr(), order.data_ptr(), lig_off.data_ptr(), bond_off.data_ptr(), B, F, cls.size(-1),
                               2 * order.size(-1), max_n, (ctypes.c_int * 4)(*(int(v) for v in limits)), out['ring_size'].data_ptr(),
                               out['atom_ring'].data_ptr(), out['ring_sys'].data_ptr(), out['counts'].data_ptr(),
                               out['status'].data_ptr(), hip.stream_ptr()), 'pg_mol_rings')


@dataclass
class Kekule:
    """Device tensors of one `kekulize` call; F frames, B graphs, N atom rows, H pair rows (as the screen's `order`)."""
    status: torch.Tensor         # int32 [F, B]     KEKULE_* bits
    counts: torch.Tensor         # int32 [F, B, 10] KEKULE_COUNTS
    ok: torch.Tensor             # bool  [F, B]     no bit of KEKULE_FAIL_MASK
    kekule_order: torch.Tensor   # int8  [F, H]     the screen's `order` with every 4 replaced by 2 or 1 (unchanged where not ok)
    hcount: torch.Tensor         # uint8 [F, N]     hydrogens of the atom; 0 for a dropped one
    charge: torch.Tensor         # int8  [F, N]     formal charge of the atom (0 or +1); 0 for a dropped one
    options: KekuleOptions
    screen: Screen               # the screen it was computed from


@torch.no_grad()
def kekulize(results, frames='final', screen=None, options=KekuleOptions()):
    """Kekulé form, hydrogens and charges of every decoded (frame, graph) of a `sample` / `sample_batch` result, on the device, in
    one launch (pg_mol_kekule; DESIGN.md 2.9 "Kekulé form"): double bonds are placed on aromatic bonds, at most one per atom, so that
    every aromatic C / Si that can still take one gets one (N, P, S may), as many as possible; first with neutral atoms only, then --
    options.allow_charged -- with N+ / P+ / S+.  `ok` is a separate answer from the screen's `valid` and the rings' `ok`: no ring
    test is applied, an aromatic bond on a chain takes part like any other.  A `Screen` of the same result and frames is reused if
    handed in.  No host read beyond the screen's.  Exact: feasibility and the number of double bonds do not depend on the numbering
    of the atoms; WHICH Kekulé structure is returned does, so this is no canonical form and nothing to build a key from.  `hydrogens -
    charge` is the same for every structure.  No tautomers, anions, O+; stereo is read afterwards, from the coordinates (`stereo`);
    not checked against RDKit."""
    node, _, edge, F, _ = _frames(results, frames)
    dev = node.device
    _need_cuda('kekulize', 'the Kekulé assignment', dev)
    if not isinstance(options, KekuleOptions):
        raise ValueError(f'phoregen_amd.molecule.kekulize: options must be a KekuleOptions, not {options!r}')
    sc = _screen_of('kekulize', screen, results, frames, F, node.size(-2), edge.size(-2), dev)
    B, N = len(sc.num_atoms), node.size(-2)
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(KEKULE_COUNTS), dtype=torch.int32, device=dev),
                   kekule_order=torch.empty(F, sc.order.size(1), dtype=torch.int8, device=dev),
                   hcount=torch.empty(F, N, dtype=torch.uint8, device=dev), charge=torch.empty(F, N, dtype=torch.int8, device=dev))
        _launch_kekule(lib, sc.cls, sc.order, sc.lig_off, sc.bond_off, B, F, max(sc.num_atoms, default=0), _kekule_table(dev),
                       bool(options.allow_charged), out)
    return Kekule(ok=(out['status'] & KEKULE_FAIL_MASK) == 0, options=options, screen=sc, **out)


def _launch_kekule(lib, cls, order, lig_off, bond_off, B, F, max_n, tables, allow_charged, out):
    """pg_mol_kekule on the current stream; tables = (DBL_NEUTRAL, DBL_CHARGED, MUST [11], H_VALENCES [11, 4]) as uint8 on the device.
    A graph above MAX_ATOMS is the library's error: nothing is launched and `out` is not written."""
    _check_arrays('kekulize', cls.device, [(cls, torch.int8), (order, torch.int8), (lig_off, torch.int32), (bond_off, torch.int32),
                                           (out['kekule_order'], torch.int8), (out['hcount'], torch.uint8), (out['charge'], torch.int8),
                                           (out['counts'], torch.int32), (out['status'], torch.int32), *((t, torch.uint8) for t in tables)])
    if (lig_off.numel() != B + 1 or bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or out['kekule_order'].shape != order.shape or out['hcount'].shape != cls.shape or out['charge'].shape != cls.shape
            or out['status'].numel() != F * B or out['counts'].numel() != len(KEKULE_COUNTS) * F * B or len(tables) != 4
            or [t.numel() for t in tables] != [len(ATOM_TYPES)] * 3 + [4 * len(ATOM_TYPES)]):
        raise ValueError(f'phoregen_amd.molecule.kekulize: sizes of the offsets, screen arrays, tables and outputs do not fit {F} frames x '
                         f'{B} graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_kekule(cls.data_ptr(), order.data_ptr(), lig_off.data_ptr(), bond_off.data_ptr(), B, F, cls.size(-1),
                                2 * order.size(-1), max_n, tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(),
                                tables[3].data_ptr(), int(bool(allow_charged)), out['kekule_order'].data_ptr(), out['hcount'].data_ptr(),
                                out['charge'].data_ptr(), out['counts'].data_ptr(), out['status'].data_ptr(), hip.stream_ptr()),
              'pg_mol_kekule')


@dataclass
class Features:
    """Device tensors of one `features` call; F frames, B graphs, N atom rows, Q = the graphs' point counts summed (graph g owns the
    columns point_off[g] .. point_off[g + 1] of the per-point tensors)."""
    status: torch.Tensor         # int32 [F, B]     FEAT_* bits
    counts: torch.Tensor         # int32 [F, B, 25] FEATURE_COUNTS
    ok: torch.Tensor             # bool  [F, B]     no bit of FEAT_FAIL_MASK
    atom_fp: torch.Tensor        # uint8 [F, N]     bit t: the atom presents FEATURE_TYPES[t]; 0 for a dropped atom
    point_dist: torch.Tensor     # fp32  [F, Q]     distance of a typed point to the nearest kept atom that carries its type (+inf: none)
    point_atom: torch.Tensor     # int16 [F, Q]     that atom's compact index (the screen's), -1: none
    point_off: torch.Tensor      # int32 [B + 1]
    point_range: torch.Tensor    # int32 [B, 2]     rows of the graph's points in the point tensors that were handed in
    point_kind: torch.Tensor     # int8  [P]        the kinds that were handed in: 0..6 = FEATURE_TYPES, -1 = untyped, -2 = ignored
    limits: FeatureLimits
    screen: Screen               # the screen it was computed from
    kekule: Kekule               # the Kekulé form it typed from
    rings: Rings                 # the rings it typed from


@torch.no_grad()
def features(results, point_pos, point_kind, point_batch=None, frames='final', screen=None, kekule=None, rings=None,
             limits=FeatureLimits()):
    """Type every atom of every decoded (frame, graph) of a `sample` / `sample_batch` result and match its pharmacophore by type, on the
    device, in one launch (pg_mol_feat; DESIGN.md 2.9 "Features").  point_pos [P, 3]: the points in the coordinates the frames hold;
    point_kind [P]: 0..6 = the index into FEATURE_TYPES of the point's type, -1 = a feature whose type is not typed (counted, never
    matched, never missed), -2 = ignored (an exclusion sphere).  point_batch as in `geometry`.  A typed point is matched iff a kept
    atom that carries its type lies closer than limits.feat_cut (strict) -- the reference's `check_nearby_phore(strict=True)`.
    Whichever of `screen`, `kekule` (a `Kekule`) and `rings` (a `Rings`) is not handed in is computed; all must come from one screen.
    No host read beyond the screen's.  `ok` is a separate answer from the other screens': with the default limits it fails only for a
    graph without a Kekulé structure or with a non-finite coordinate.  The rules are written from the reference's SMARTS text and not
    checked against RDKit; `arom` is the model's bond class on a ring bond, not RDKit's perception; MB, CV1..CV4 and CR are not typed;
    atom positions are used, not ring centroids, as in the reference's own check."""
    node, pos, edge, F, (_, _, pos_fs) = _frames(results, frames)
    dev = pos.device
    _need_cuda('features', 'the feature typing', dev)
    if not isinstance(limits, FeatureLimits):
        raise ValueError(f'phoregen_amd.molecule.features: limits must be a FeatureLimits, not {limits!r}')
    P = _point_count('features', point_pos)
    if not torch.is_tensor(point_kind) or point_kind.numel() != P or point_kind.dtype.is_floating_point or point_kind.dtype == torch.bool:
        raise ValueError(f'phoregen_amd.molecule.features: {P} points, point_kind must hold one integer kind per point, it has '
                         f'{getattr(point_kind, "shape", None)} of {getattr(point_kind, "dtype", None)}')
    sc = _resolve('features', results, frames, screen, kekule=kekule, rings=rings)
    B, N = len(sc.num_atoms), pos.size(-2)
    _check_rows('features', pos, F, 3, 'coordinates', dev)
    kek = kekule if kekule is not None else _kekulize(results, frames, screen=sc)
    rg = rings if rings is not None else _rings(results, frames, screen=sc)
    with torch.cuda.device(dev):
        lib = hip.lib()
        ranges, off, Q, ppos = _points(point_pos, point_batch, B, dev)
        pk = point_kind.reshape(-1).to(dev)
        pk = torch.where((pk >= POINT_UNTYPED) & (pk < len(FEATURE_TYPES)), pk, torch.full_like(pk, POINT_IGNORED)).to(torch.int8)
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(FEATURE_COUNTS), dtype=torch.int32, device=dev),
                   atom_fp=torch.empty(F, N, dtype=torch.uint8, device=dev), point_dist=torch.empty(F, Q, dtype=torch.float32, device=dev),
                   point_atom=torch.empty(F, Q, dtype=torch.int16, device=dev))
        _launch_feat(lib, pos, pos_fs, sc, kek, rg, B, F, max(sc.num_atoms, default=0), ppos, pk, ranges, off, Q, limits, out)
    return Features(ok=(out['status'] & FEAT_FAIL_MASK) == 0, point_off=off, point_range=ranges, point_kind=pk, limits=limits, screen=sc,
                    kekule=kek, rings=rg, **out)


def point_kinds_of(x, type_names, ex_name='EX'):
    """int8 [P] point kinds of one-hot pharmacophore rows x [P, >= len(type_names)]: the argmax over the first len(type_names) columns,
    mapped by name -- a name of FEATURE_TYPES to its index, `ex_name` to -2 (ignored), any other name to -1 (untyped)."""
    table = torch.tensor([FEATURE_TYPES.index(t) if t in FEATURE_TYPES else POINT_IGNORED if t == ex_name else POINT_UNTYPED
                          for t in type_names], dtype=torch.int8, device=x.device)
    if x.size(0) == 0:
        return torch.zeros(0, dtype=torch.int8, device=x.device)
    return table[x[:, :len(type_names)].argmax(-1)]


def features_for(data, results, frames='final', screen=None, kekule=None, rings=None, limits=FeatureLimits(), type_names=None):
    """`features` with the pharmacophore of `data` as `PhoreDiff.sample` reads it: the points are data['phore'].pos + data.center, as in
    `geometry_for`; a point's type is the argmax over the first len(type_names) columns of data['phore'].x, by name (type_names
    defaults to data.PHORETYPES1, the zinc_300 / pdbbind order; 'EX' rows are ignored, names outside FEATURE_TYPES are untyped);
    every graph has all points."""
    if type_names is None:
        from .data import PHORETYPES1
        type_names = PHORETYPES1
    ph = data['phore']
    return features(results, ph.pos.float() + data.center.to(ph.pos.device).float(), point_kinds_of(ph.x, type_names), None, frames,
                    screen, kekule, rings, limits)


def _launch_feat(lib, pos, pos_fs, sc, kek, rg, B, F, max_n, point_pos, point_kind, ranges, off, n_out, limits, out):
    """pg_mol_feat on the current stream; sc, kek, rg: anything with the `Screen`, `Kekule` and `Rings` fields the kernel reads.  A graph
    above MAX_ATOMS is the library's error: nothing is launched and `out` is not written."""
    cls, order = sc.cls, sc.order
    _check_arrays('features', pos.device, [
        (cls, torch.int8), (order, torch.int8), (sc.compact, torch.int16), (kek.kekule_order, torch.int8), (kek.hcount, torch.uint8),
        (kek.charge, torch.int8), (kek.status, torch.int32), (rg.ring_size, torch.uint8), (sc.lig_off, torch.int32), (sc.bond_off, torch.int32),
        (point_pos, torch.float32), (point_kind, torch.int8), (ranges, torch.int32), (off, torch.int32), (out['atom_fp'], torch.uint8),
        (out['point_dist'], torch.float32), (out['point_atom'], torch.int16), (out['counts'], torch.int32), (out['status'], torch.int32)])
    if (sc.lig_off.numel() != B + 1 or sc.bond_off.numel() != B + 1 or off.numel() != B + 1 or ranges.numel() != 2 * B
            or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1) or pos.size(-2) != cls.size(-1)
            or sc.compact.shape != cls.shape or kek.hcount.shape != cls.shape or kek.charge.shape != cls.shape
            or kek.kekule_order.shape != order.shape or rg.ring_size.shape != order.shape or kek.status.numel() != F * B
            or point_kind.numel() != point_pos.size(0) or out['atom_fp'].shape != cls.shape
            or tuple(out['point_dist'].shape) != (F, n_out) or tuple(out['point_atom'].shape) != (F, n_out)
            or out['status'].numel() != F * B or out['counts'].numel() != len(FEATURE_COUNTS) * F * B):
        raise ValueError('phoregen_amd.molecule.features: sizes of the offsets, ranges, screen / Kekulé / ring arrays, points and outputs do '
                         f'not fit {F} frames x {B} graphs, {cls.size(-1)} atom rows, {point_pos.size(0)} points, {n_out} point outputs')
    hip.check(lib.pg_mol_feat(pos.data_ptr(), pos_fs, cls.data_ptr(), order.data_ptr(), sc.compact.data_ptr(), kek.kekule_order.data_ptr(),
                              kek.hcount.data_ptr(), kek.charge.data_ptr(), kek.status.data_ptr(), rg.ring_size.data_ptr(),
                              sc.lig_off.data_ptr(), sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1), max_n,
                              point_pos.data_ptr(), point_kind.data_ptr(), point_pos.size(0), ranges.data_ptr(), off.data_ptr(), n_out,
                              float(limits.feat_cut), int(limits.max_unmatched), out['atom_fp'].data_ptr(), out['point_dist'].data_ptr(),
                              out['point_atom'].data_ptr(), out['counts'].data_ptr(), out['status'].data_ptr(), hip.stream_ptr()),
              'pg_mol_feat')


@dataclass
class Stereo:
    """Device tensors of one `stereo` call; F frames, B graphs, N atom rows, H pair rows (as the screen's `order`).  Values: 0 = not
    stereogenic, +1 / -1, 2 = stereogenic but undefined."""
    status: torch.Tensor         # int32 [F, B]     STEREO_* bits
    counts: torch.Tensor         # int32 [F, B, 8]  STEREO_COUNTS
    ok: torch.Tensor             # bool  [F, B]     no bit of STEREO_FAIL_MASK
    atom_parity: torch.Tensor    # int8  [F, N]     sign of the centre's signed volume with its neighbours in index order
    atom_label: torch.Tensor     # int8  [F, N]     the parity with the neighbours in colour order: independent of the numbering
    bond_stereo: torch.Tensor    # int8  [F, H]     +1 cis / -1 trans of the lowest-index substituents of the pair's double bond
    bond_label: torch.Tensor     # int8  [F, H]     the same of the largest-colour substituents: independent of the numbering
    stereo_key: torch.Tensor     # int64 [F, B]     the identity key with the defined labels mixed in (the key itself without any)
    limits: StereoLimits
    screen: Screen               # the screen it was computed from
    kekule: Kekule               # the Kekulé form, the rings and the keys it was computed from
    rings: Rings
    keys: MolKeys


@torch.no_grad()
def stereo(results, frames='final', screen=None, kekule=None, rings=None, keys=None, limits=StereoLimits()):
    """Stereo perception of every decoded (frame, graph) of a `sample` / `sample_batch` result from its coordinates, on the device,
    in one launch (pg_mol_stereo; DESIGN.md 2.9 "Stereo").  Centres: C, N, Si, P, S with four heavy neighbours, or three and one
    hydrogen, whose heavy neighbours all differ in colour (`molecule_keys`); the parity is the sign of the signed volume of the unit
    vectors to the neighbours in index order (the hydrogen opposite the other three), if it reaches limits.vol_min.  Double bonds:
    Kekulé order 2, not aromatic, in no ring, neither end with another multiple bond, every end with two substituents of different
    colour or with one and at most one hydrogen; cis / trans of the lowest-index substituents, if the planarity measure reaches
    limits.planar_min.  The labels restate both relative to the colours, so they -- and `stereo_key` -- do not depend on the numbering
    of the atoms as far as atoms with equal colours are in fact equivalent (the identity key's own stance); a reflection flips every
    atom label, leaves the bond labels and changes the key of a chiral molecule but not of a meso one.  Whichever of `screen`,
    `kekule`, `rings` and `keys` (a `MolKeys`) is not handed in is computed; all must come from one screen.  No host read beyond the
    screen's.  `ok` fails without a Kekulé structure, with a non-finite coordinate, or with more than limits.max_undefined undefined
    elements.  No R / S or E / Z names, no pseudo-asymmetric centres, no ring double bonds, allenes or atropisomers; three-coordinate
    N, P and S are never centres; the thresholds are design choices, not calibrated; not checked against RDKit."""
    node, pos, edge, F, (_, _, pos_fs) = _frames(results, frames)
    dev = pos.device
    _need_cuda('stereo', 'the stereo perception', dev)
    if not isinstance(limits, StereoLimits):
        raise ValueError(f'phoregen_amd.molecule.stereo: limits must be a StereoLimits, not {limits!r}')
    sc = _resolve('stereo', results, frames, screen, kekule=kekule, rings=rings, keys=keys)
    _check_rows('stereo', pos, F, 3, 'coordinates', dev)
    kek = kekule if kekule is not None else _kekulize(results, frames, screen=sc)
    rg = rings if rings is not None else _rings(results, frames, screen=sc)
    mk = keys if keys is not None else molecule_keys(sc)
    B, N = len(sc.num_atoms), pos.size(-2)
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(STEREO_COUNTS), dtype=torch.int32, device=dev),
                   atom_parity=torch.empty(F, N, dtype=torch.int8, device=dev), atom_label=torch.empty(F, N, dtype=torch.int8, device=dev),
                   bond_stereo=torch.empty(F, sc.order.size(1), dtype=torch.int8, device=dev),
                   bond_label=torch.empty(F, sc.order.size(1), dtype=torch.int8, device=dev),
                   stereo_key=torch.empty(F, B, dtype=torch.int64, device=dev))
        _launch_stereo(lib, pos, pos_fs, sc, kek, rg, mk, B, F, max(sc.num_atoms, default=0), limits, out)
    return Stereo(ok=(out['status'] & STEREO_FAIL_MASK) == 0, limits=limits, screen=sc, kekule=kek, rings=rg, keys=mk, **out)


def _launch_stereo(lib, pos, pos_fs, sc, kek, rg, mk, B, F, max_n, limits, out):
    """pg_mol_stereo on the current stream; sc, kek, rg, mk: anything with the `Screen`, `Kekule`, `Rings` and `MolKeys` fields the kernel
    reads.  A graph above MAX_ATOMS is the library's error: nothing is launched and `out` is not written."""
    cls, order = sc.cls, sc.order
    _check_arrays('stereo', pos.device, [
        (cls, torch.int8), (order, torch.int8), (kek.kekule_order, torch.int8), (kek.hcount, torch.uint8), (kek.charge, torch.int8),
        (kek.status, torch.int32), (rg.ring_size, torch.uint8), (mk.colour, torch.int64), (mk.key, torch.int64), (sc.lig_off, torch.int32),
        (sc.bond_off, torch.int32), (out['atom_parity'], torch.int8), (out['atom_label'], torch.int8), (out['bond_stereo'], torch.int8),
        (out['bond_label'], torch.int8), (out['stereo_key'], torch.int64), (out['counts'], torch.int32), (out['status'], torch.int32)])
    if (sc.lig_off.numel() != B + 1 or sc.bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or pos.size(-2) != cls.size(-1) or pos.dtype != torch.float32 or pos.device != cls.device
            or kek.hcount.shape != cls.shape or kek.charge.shape != cls.shape or kek.kekule_order.shape != order.shape
            or rg.ring_size.shape != order.shape or kek.status.numel() != F * B or mk.colour.shape != cls.shape or mk.key.numel() != F * B
            or out['atom_parity'].shape != cls.shape or out['atom_label'].shape != cls.shape or out['bond_stereo'].shape != order.shape
            or out['bond_label'].shape != order.shape or out['stereo_key'].numel() != F * B or out['status'].numel() != F * B
            or out['counts'].numel() != len(STEREO_COUNTS) * F * B):
        raise ValueError('phoregen_amd.molecule.stereo: sizes of the offsets, screen / Kekulé / ring / key arrays and outputs do not fit '
                         f'{F} frames x {B} graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows')
    hip.check(lib.pg_mol_stereo(pos.data_ptr(), pos_fs, cls.data_ptr(), order.data_ptr(), kek.kekule_order.data_ptr(), kek.hcount.data_ptr(),
                                kek.charge.data_ptr(), kek.status.data_ptr(), rg.ring_size.data_ptr(), mk.colour.data_ptr(),
                                mk.key.data_ptr(), sc.lig_off.data_ptr(), sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1),
                                max_n, float(limits.vol_min), float(limits.planar_min), int(limits.max_undefined),
                                out['atom_parity'].data_ptr(), out['atom_label'].data_ptr(), out['bond_stereo'].data_ptr(),
                                out['bond_label'].data_ptr(), out['stereo_key'].data_ptr(), out['counts'].data_ptr(),
                                out['status'].data_ptr(), hip.stream_ptr()), 'pg_mol_stereo')


@dataclass
class Smiles:
    """Device tensors of one `smiles` call; F frames, B graphs, N atom rows."""
    status: torch.Tensor         # int32 [F, B]     SMILES_* bits
    counts: torch.Tensor         # int32 [F, B, 8]  SMILES_COUNTS
    ok: torch.Tensor             # bool  [F, B]     no bit of SMILES_FAIL_MASK
    text: torch.Tensor           # uint8 [F, B, capacity]  ASCII, zeros from `length` on
    length: torch.Tensor         # int32 [F, B]     bytes of text; 0 where not ok
    atom_rank: torch.Tensor      # int16 [F, N]     position of the atom in the text, -1 = dropped (or not ok)
    capacity: int
    screen: Screen               # the screen it was written from
    kekule: Kekule               # the Kekulé form it was written from
    stereo_counts: torch.Tensor = None   # int32 [F, B, 4]  SMILES_STEREO_COUNTS; None unless written with stereo=
    stereo: Stereo = None        # the stereo it was written with

    def strings(self, frame=0):
        """The texts of one frame as a list of str, one per graph ('' where not ok), from one device-to-host copy."""
        B, cap = self.text.size(1), self.capacity
        blob = torch.cat([self.length[frame].reshape(-1).view(torch.uint8), self.text[frame].reshape(-1)]).cpu().numpy()
        length, text = blob[:4 * B].view(np.int32), blob[4 * B:]
        return [text[g * cap:g * cap + int(length[g])].tobytes().decode('ascii') for g in range(B)]


@torch.no_grad()
def smiles(results, frames='final', screen=None, kekule=None, capacity=None, stereo=None):
    """SMILES text of every decoded (frame, graph) of a `sample` / `sample_batch` result, on the device, in one launch (pg_mol_smiles;
    DESIGN.md 2.9 "SMILES"): Kekulé-form OpenSMILES of the kept atoms with the Kekulé form's bond orders, hydrogens and charges --
    depth-first from the lowest atom not yet written, neighbours ascending, ring-closure labels 1..99, '=' and '#', bracket atoms
    where a bare symbol would not read back with the atom's hydrogens and charge, components joined by '.'.  Whichever of `screen`
    and `kekule` (a `Kekule`) is not handed in is computed; both must come from one screen.  capacity: bytes of a text row, None =
    8 * max(largest graph, 8); a text that needs more is SMILES_TOO_LONG, with the need in the count 'length'.  No host read beyond
    the screen's.  `ok` fails for a graph without a Kekulé structure, with more than 99 labels in use at once or with too long a
    text.  The text reads back to exactly the molecule `assemble` returns (`atom_rank`: where each atom stands in it); it is NOT
    canonical -- the numbering of the atoms and the choice of Kekulé structure both change it, identity stays with `molecule_keys` --
    and has no aromatic lower-case form, no anions; not checked against RDKit.
    stereo=a `Stereo` of the same screen: the text is isomeric (pg_mol_smiles_stereo; DESIGN.md 2.9 "Stereo") -- a centre with parity
    +1 / -1 is a bracket atom with '@' or '@@', the single bonds next to a cis / trans double bond are '/' or '\\'; undefined
    elements are written without a mark.  The Kekulé form is the stereo's unless one is handed in; capacity None = 12 * max(largest
    graph, 8); `stereo_counts` holds SMILES_STEREO_COUNTS.  Without stereo= the text has no stereo and `stereo_counts` is None; with
    a `Stereo` that has no +1 / -1 the text is the same byte for byte."""
    node, _, edge, F, _ = _frames(results, frames)
    dev = node.device
    _need_cuda('smiles', 'the SMILES writer', dev)
    if stereo is not None and not isinstance(stereo, Stereo):
        raise ValueError(f'phoregen_amd.molecule.smiles: stereo= must be a Stereo, not {stereo!r}')
    sc = _resolve('smiles', results, frames, screen, kekule=kekule, stereo=stereo)
    kek = kekule if kekule is not None else stereo.kekule if stereo is not None else _kekulize(results, frames, screen=sc)
    B, N, max_n = len(sc.num_atoms), node.size(-2), max(sc.num_atoms, default=0)
    cap = _check_int('phoregen_amd.molecule.smiles', 'capacity', (8 if stereo is None else 12) * max(max_n, 8) if capacity is None else capacity,
                     1, 0x7fffffff)
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(SMILES_COUNTS), dtype=torch.int32, device=dev),
                   text=torch.empty(F, B, int(cap), dtype=torch.uint8, device=dev), length=torch.empty(F, B, dtype=torch.int32, device=dev),
                   atom_rank=torch.empty(F, N, dtype=torch.int16, device=dev))
        if stereo is not None:
            out['stereo_counts'] = torch.empty(F, B, len(SMILES_STEREO_COUNTS), dtype=torch.int32, device=dev)
        _launch_smiles(lib, sc, kek, B, F, max_n, _smiles_table(dev), int(cap), out, stereo)
    return Smiles(ok=(out['status'] & SMILES_FAIL_MASK) == 0, capacity=int(cap), screen=sc, kekule=kek, stereo=stereo, **out)


def _launch_smiles(lib, sc, kek, B, F, max_n, table, capacity, out, st=None):
    """pg_mol_smiles -- with st, anything with the `Stereo` fields atom_parity and bond_stereo, pg_mol_smiles_stereo, and `out` then
    has 'stereo_counts' -- on the current stream; sc, kek: anything with the `Screen` and `Kekule` fields the kernel reads; table =
    SMILES_VALENCES [11, 4] as uint8 on the device.  A graph above MAX_ATOMS is the library's error: nothing is launched and `out` is
    not written."""
    cls, order = sc.cls, kek.kekule_order
    _check_arrays('smiles', cls.device, [(cls, torch.int8), (order, torch.int8), (kek.hcount, torch.uint8), (kek.charge, torch.int8),
                                         (kek.status, torch.int32), (sc.lig_off, torch.int32), (sc.bond_off, torch.int32),
                                         (table, torch.uint8), (out['text'], torch.uint8), (out['length'], torch.int32),
                                         (out['atom_rank'], torch.int16), (out['counts'], torch.int32), (out['status'], torch.int32)])
    if (sc.lig_off.numel() != B + 1 or sc.bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or order.shape != sc.order.shape or kek.hcount.shape != cls.shape or kek.charge.shape != cls.shape
            or kek.status.numel() != F * B or table.numel() != 4 * len(ATOM_TYPES) or out['text'].numel() != F * B * capacity
            or out['length'].numel() != F * B or out['atom_rank'].shape != cls.shape or out['status'].numel() != F * B
            or out['counts'].numel() != len(SMILES_COUNTS) * F * B):
        raise ValueError(f'phoregen_amd.molecule.smiles: sizes of the offsets, screen / Kekulé arrays, table and outputs do not fit {F} '
                         f'frames x {B} graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows, capacity {capacity}')
    if st is not None:
        _check_arrays('smiles', cls.device, [(st.atom_parity, torch.int8), (st.bond_stereo, torch.int8), (out['stereo_counts'], torch.int32)])
        if (st.atom_parity.shape != cls.shape or st.bond_stereo.shape != order.shape
                or out['stereo_counts'].numel() != len(SMILES_STEREO_COUNTS) * F * B):
            raise ValueError(f'phoregen_amd.molecule.smiles: sizes of the stereo arrays do not fit {F} frames x {B} graphs, {cls.size(-1)} '
                             f'atom rows, {order.size(-1)} pair rows')
        hip.check(lib.pg_mol_smiles_stereo(cls.data_ptr(), order.data_ptr(), kek.hcount.data_ptr(), kek.charge.data_ptr(),
                                           kek.status.data_ptr(), st.atom_parity.data_ptr(), st.bond_stereo.data_ptr(),
                                           sc.lig_off.data_ptr(), sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1), max_n,
                                           table.data_ptr(), capacity, out['text'].data_ptr(), out['length'].data_ptr(),
                                           out['atom_rank'].data_ptr(), out['counts'].data_ptr(), out['status'].data_ptr(),
                                           out['stereo_counts'].data_ptr(), hip.stream_ptr()), 'pg_mol_smiles_stereo')
        return
    hip.check(lib.pg_mol_smiles(cls.data_ptr(), order.data_ptr(), kek.hcount.data_ptr(), kek.charge.data_ptr(), kek.status.data_ptr(),
                                sc.lig_off.data_ptr(), sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1), max_n,
                                table.data_ptr(), capacity, out['text'].data_ptr(), out['length'].data_ptr(),
                                out['atom_rank'].data_ptr(), out['counts'].data_ptr(), out['status'].data_ptr(), hip.stream_ptr()),
              'pg_mol_smiles')


def formula_of(elements, hcount, charge=0):
    """Molecular formula in Hill order (C, H, then the other symbols alphabetically; all alphabetically without carbon) from atomic
    numbers and per-atom hydrogen counts, with a charge suffix such as '+' / '2+' / '-', and the molecular weight from ATOMIC_WEIGHT
    (standard atomic weights, written from memory)."""
    n = {}
    for z in elements:
        n[ELEMENT_SYMBOL[int(z)]] = n.get(ELEMENT_SYMBOL[int(z)], 0) + 1
    n_h = int(np.asarray(hcount, dtype=np.int64).sum())
    weight = sum(ATOMIC_WEIGHT[int(z)] for z in elements) + n_h * ATOMIC_WEIGHT[1]
    if n_h:
        n['H'] = n_h
    first = [k for k in ('C', 'H') if k in n] if 'C' in n else []
    text = ''.join(k + (str(n[k]) if n[k] > 1 else '') for k in first + sorted(k for k in n if k not in first))
    q = int(charge)
    if q:
        text += (str(abs(q)) if abs(q) > 1 else '') + ('+' if q > 0 else '-')
    return text, float(weight)


_geometry = geometry             # (functions below take a `geometry=` argument)
_rings = rings                   # (and a `rings=` argument)
_kekulize = kekulize
_features = features
_smiles = smiles
_stereo = stereo
_fingerprints = fingerprints


@lru_cache(maxsize=None)
def _pairs(n):
    """The pairs a < b of n atoms in row-major order: the first half of a graph's bond rows (plan.make_edge_data).  Kept per n."""
    a, b = np.triu_indices(n, 1)
    return a.astype(np.int64), b.astype(np.int64)


# ---- carriers: what `assemble`, `write_sdf` and `sample_valid` know about each analysis ------------------------------------------------
@dataclass(frozen=True)
class _Analysis:
    """One analysis of the decoded molecules as the three carrying functions see it.  A further analysis is one more record in
    _ANALYSES_SINCE, its keyword in the signatures of `assemble` and `sample_valid`, and a paragraph in their docstrings."""
    keyword: str                 # its keyword of `assemble` and `sample_valid`
    key: str                     # the key a molecule that carries it has (the first one, if it adds several)
    holder: type                 # what `assemble` is handed: a dataclass of device tensors with a `screen`
    parts: object                # holder -> [(name, final-frame tensor, numpy dtype)]: its parts of the blob; names are the views' keys
    entry: object                # (holder, views, _MolView, the molecule so far) -> the entries it adds to the molecule's dict
    sdf: object                  # molecule -> the text of its data item of `write_sdf`
    read: object                 # `sample_valid`'s argument -> what `compute` takes (True: the defaults), None: not asked for; ValueError
    compute: object              # (_Draw, what `read` gave) -> the holder of a draw
    verdict: object = None       # molecule -> bool, what `sample_valid` filters on; None: nothing
    frames: str = 'status'       # a tensor of the holder with the frames as its first dimension
    also: tuple = ()             # keywords of the analyses `sample_valid` carries, and filters on, along with it


def _analyses(want, among=None):
    """The records of the entries of _ANALYSES (or of the list `among`) that `want` accepts (it sees `keyword` and `key`), in the
    list's order.  An entry that is no record stands for the ANALYSIS of phoregen_amd.<keyword>, which is loaded here: only for a
    caller who asks for it."""
    return [a if isinstance(a, _Analysis) else import_module('.' + a.keyword, __package__).ANALYSIS
            for a in (_ANALYSES if among is None else among) if want(a)]


def _carried(want):
    """`_analyses` over everything the three carrying functions know: _ANALYSES, then _ANALYSES_SINCE."""
    return _analyses(want, _ANALYSES + _ANALYSES_SINCE)


def _handed(args):
    """[(record, value)] of the analyses whose keyword has a value in `args`, in the list's order."""
    return [(rec, args[rec.keyword]) for rec in _carried(lambda a: args.get(a.keyword) is not None)]


class _MolView(namedtuple('_MolView', 'g n0 n keep h0 h nz cmp_g')):
    """Where graph g lies in the host views of `assemble` -- its atom rows n0 .. n0 + n and which were kept (keep, bool [n]), its pair
    rows h0 .. h0 + h and which, counted from h0, are bonds (nz), its atoms' indices among the kept ones (cmp_g, int64 [n], -1 =
    dropped) -- and the slicings its entries are made of."""

    def atoms(self, a):                                                # the rows of the kept atoms of a per-atom view
        return a[self.n0:self.n0 + self.n][self.keep]

    def bonds(self, a):                                                # the entries of the bonds of a per-pair view, in 'bond_type's order
        return a[self.h0:self.h0 + self.h][self.nz]

    def row(self, a):                                                  # the graph's row of a per-graph view
        return a[self.g]

    def points(self, a, off):                                          # the graph's points off[g] .. off[g + 1] of a per-point view
        return a[int(off[self.g]):int(off[self.g + 1])]


def _status_entry(ok_key, mask, names, status, counts):
    """How an analysis's dict begins: 'status', its verdict (no bit of `mask`) and the counts by name."""
    return dict({'status': int(status), ok_key: (int(status) & mask) == 0}, **{k: int(x) for k, x in zip(names, counts)})


def _true_or(keyword, cls=None):
    """The reader of a `sample_valid` argument that is True (the defaults) or a `cls`; without a `cls`, True and nothing else."""
    def read(value):
        opt = cls() if cls and value is True else value
        if not (isinstance(opt, cls) if cls else opt is True):
            raise ValueError(f'phoregen_amd.molecule.sample_valid: {keyword}= must be True{f" or a {cls.__name__}" if cls else ""}, not {value!r}')
        return opt
    return read


def _geom_entry(x, v, at, mol):
    return {'geom': dict(_status_entry('geom_ok', GEOM_FAIL_MASK, (), at.row(v['g_status']), ()),
                         **{k: float(a) for k, a in zip(GEOM_METRICS, at.row(v['g_metrics']))},
                         **{k: int(a) for k, a in zip(GEOM_COUNTS, at.row(v['g_counts']))},
                         point_dist=at.points(v['g_dist'], v['g_off']).copy(), point_atom=at.points(v['g_atom'], v['g_off']).copy())}


def _rings_entry(x, v, at, mol):
    sys_g = at.atoms(v['r_sys']).astype(np.int64)                      # local index of the system's first atom -> its compact index
    return {'rings': dict(_status_entry('rings_ok', RING_FAIL_MASK, RING_COUNTS, at.row(v['r_status']), at.row(v['r_counts'])),
                          bond_ring_size=at.bonds(v['r_size']).copy(), atom_ring=at.atoms(v['r_atom']).copy(),
                          ring_sys=np.where(sys_g >= 0, at.cmp_g[np.maximum(sys_g, 0)], -1).astype(np.int16))}


def _kekule_entry(x, v, at, mol):
    k_h, k_q = at.atoms(v['k_h']).copy(), at.atoms(v['k_q']).copy()
    formula, weight = formula_of(mol['element'], k_h, int(k_q.astype(np.int64).sum()))
    return {'kekule': dict(_status_entry('kekule_ok', KEKULE_FAIL_MASK, _KEKULE_KEYS.values(), at.row(v['k_status']), at.row(v['k_counts'])),
                           bond_type=torch.from_numpy(at.bonds(v['k_order']).astype(np.int64)), hcount=k_h, charge=k_q,
                           formula=formula, mol_weight=weight)}


def _features_entry(x, v, at, mol):
    fp, (lo, hi) = at.atoms(v['f_fp']).copy(), at.row(v['f_range'])
    ft = dict(_status_entry('features_ok', FEAT_FAIL_MASK, FEATURE_COUNTS, at.row(v['f_status']), at.row(v['f_counts'])), atom_fp=fp,
              atom_types=[_TYPES_OF_BYTE[b] for b in fp.tolist()],
              point_kind=v['f_kind'][int(lo):int(hi)].copy(),
              point_dist=at.points(v['f_dist'], v['f_off']).copy(), point_atom=at.points(v['f_atom'], v['f_off']).copy())
    # (the kernel's own comparison: fp32 distance < fp32 cutoff; a non-finite point has distance +inf)
    ft['point_matched'] = ft['point_dist'] < np.float32(x.limits.feat_cut)
    return {'features': ft}


def _features_item(ft):
    """The PHOREGEN_FEATURES data item of a molecule's 'features' dict (`assemble`)."""
    lines = ['> <PHOREGEN_FEATURES>', 'status 0x%02x' % int(ft['status'])] + ['%s %d' % (k, ft[k]) for k in FEATURE_COUNTS]
    kinds = np.asarray(ft['point_kind']).reshape(-1).tolist()
    dist, atom = np.asarray(ft['point_dist']).reshape(-1).tolist(), np.asarray(ft['point_atom']).reshape(-1).tolist()
    for k, d, a, hit in zip(kinds, dist, atom, np.asarray(ft['point_matched']).reshape(-1).tolist()):
        if 0 <= k < len(FEATURE_TYPES):
            lines.append('%s %s %s' % (FEATURE_TYPES[k], str(a + 1) if hit else '-', '%.4f' % d if np.isfinite(d) else 'inf'))
    return '\n'.join(lines) + '\n\n'


def _read_features(value):
    if value is not True and not (isinstance(value, tuple) and len(value) == 3 and isinstance(value[2], FeatureLimits)):
        raise ValueError(f'phoregen_amd.molecule.sample_valid: features= must be True or (point_pos, point_kind, FeatureLimits), not {value!r}')
    return value


def _smiles_entry(x, v, at, mol):
    sm = _status_entry('smiles_ok', SMILES_FAIL_MASK, (), at.row(v['s_status']), ())
    sm['text'] = at.row(v['s_text'])[:int(at.row(v['s_length']))].tobytes().decode('ascii') if sm['smiles_ok'] else ''
    sm.update({k: int(a) for k, a in zip(SMILES_COUNTS, at.row(v['s_counts']))}, atom_rank=at.atoms(v['s_rank']).copy())
    if x.stereo_counts is not None:
        sm.update({k: int(a) for k, a in zip(SMILES_STEREO_COUNTS, at.row(v['s_stereo']))})
    return {'smiles': sm}


def _stereo_item(m):
    """The PHOREGEN_STEREO data item of a molecule that carries 'stereo' (`assemble`)."""
    st, sign = m['stereo'], {1: '+', -1: '-', STEREO_UNDEFINED_VALUE: '?'}
    lines = ['> <PHOREGEN_STEREO>', 'status 0x%02x' % int(st['status']), 'stereo_key %016x' % (int(st['stereo_key']) & _M64)]
    lines += ['%s %d' % (k, st[k]) for k in STEREO_COUNTS]
    for i, (p, l) in enumerate(zip(np.asarray(st['atom_parity']).tolist(), np.asarray(st['atom_label']).tolist())):
        if p:
            lines.append('centre %d %s %s' % (i + 1, sign[p], sign[l]))
    bi = np.asarray(m['bond_index']).reshape(2, -1)
    for (a, b), p, l in zip(bi.T.tolist(), np.asarray(st['bond_stereo']).tolist(), np.asarray(st['bond_label']).tolist()):
        if p:
            lines.append('bond %d %d %s %s' % (a + 1, b + 1, sign[p], sign[l]))
    return '\n'.join(lines) + '\n\n'


def _fingerprint_item(m):
    """The PHOREGEN_FINGERPRINT data item of a molecule that carries 'fingerprint' (`assemble`)."""
    words = [int(w) & _M64 for w in np.asarray(m['fingerprint']).reshape(-1).tolist()]
    if len(words) != FP_WORDS:
        raise ValueError(f"write_sdf: 'fingerprint' has {len(words)} words, not {FP_WORDS}")
    return '> <PHOREGEN_FINGERPRINT>\n%s\nradius %d\n\n' % (''.join('%016x' % w for w in words), int(m.get('fp_radius', FP_RADIUS)))


# The analyses in the order their keys stand in a molecule's dict, which is also the order of their data items in an SDF record
_ANALYSES = [
    _Analysis('geometry', 'geom', Geometry,
              parts=lambda x: [('g_status', x.status[0], np.int32), ('g_metrics', x.metrics[0], np.float32), ('g_counts', x.counts[0], np.int32),
                               ('g_dist', x.point_dist[0], np.float32), ('g_off', x.point_off, np.int32), ('g_atom', x.point_atom[0], np.int16)],
              entry=_geom_entry, read=lambda value: value, verdict=lambda m: m['geom']['geom_ok'],
              sdf=lambda m: '> <PHOREGEN_GEOM>\nstatus 0x%02x\n' % int(m['geom']['status'])
              + ''.join('%s %.4f\n' % (k, m['geom'][k]) for k in GEOM_METRICS[:7]) + '\n',
              compute=lambda d, opt: (geometry_for(d.data, d.res, screen=d.screen, ex_col=getattr(d.model, 'ex_col', 12)) if opt is True
                                      else _geometry(d.res, opt[0], opt[1], screen=d.screen, limits=opt[2]))),
    _Analysis('rings', 'rings', Rings,
              parts=lambda x: [('r_status', x.status[0], np.int32), ('r_counts', x.counts[0], np.int32), ('r_sys', x.ring_sys[0], np.int16),
                               ('r_atom', x.atom_ring[0], np.uint8), ('r_size', x.ring_size[0], np.uint8)],
              entry=_rings_entry, read=_true_or('rings', RingLimits), verdict=lambda m: m['rings']['rings_ok'],
              sdf=lambda m: '> <PHOREGEN_RINGS>\nstatus 0x%02x\n' % int(m['rings']['status'])
              + ''.join('%s %d\n' % (k, m['rings'][k]) for k in RING_COUNTS) + '\n',
              compute=lambda d, opt: _rings(d.res, screen=d.screen, limits=opt)),
    _Analysis('kekule', 'kekule', Kekule,
              parts=lambda x: [('k_status', x.status[0], np.int32), ('k_counts', x.counts[0], np.int32), ('k_order', x.kekule_order[0], np.int8),
                               ('k_h', x.hcount[0], np.uint8), ('k_q', x.charge[0], np.int8)],
              entry=_kekule_entry, read=_true_or('kekule', KekuleOptions), verdict=lambda m: m['kekule']['kekule_ok'],
              sdf=lambda m: '> <PHOREGEN_KEKULE>\nstatus 0x%02x\nformula %s\nmol_weight %.3f\n'
              % (int(m['kekule']['status']), m['kekule']['formula'], m['kekule']['mol_weight'])
              + ''.join('%s %d\n' % (k, m['kekule'][_KEKULE_KEYS[k]]) for k in KEKULE_COUNTS) + '\n',
              compute=lambda d, opt: _kekulize(d.res, screen=d.screen, options=opt)),
    _Analysis('features', 'features', Features,
              parts=lambda x: [('f_status', x.status[0], np.int32), ('f_counts', x.counts[0], np.int32), ('f_dist', x.point_dist[0], np.float32),
                               ('f_off', x.point_off, np.int32), ('f_range', x.point_range, np.int32), ('f_atom', x.point_atom[0], np.int16),
                               ('f_fp', x.atom_fp[0], np.uint8), ('f_kind', x.point_kind, np.int8)],
              entry=_features_entry, sdf=lambda m: _features_item(m['features']), read=_read_features, verdict=lambda m: m['features']['features_ok'],
              compute=lambda d, opt: (features_for(d.data, d.res, screen=d.screen, kekule=d.of('kekule'), rings=d.of('rings')) if opt is True
                                      else _features(d.res, opt[0], opt[1], screen=d.screen, kekule=d.of('kekule'), rings=d.of('rings'), limits=opt[2]))),
    _Analysis('smiles', 'smiles', Smiles,
              parts=lambda x: [('s_status', x.status[0], np.int32), ('s_counts', x.counts[0], np.int32), ('s_length', x.length[0], np.int32),
                               ('s_rank', x.atom_rank[0], np.int16), ('s_text', x.text[0], np.uint8)]
              + ([] if x.stereo_counts is None else [('s_stereo', x.stereo_counts[0], np.int32)]),
              entry=_smiles_entry, read=_true_or('smiles'),
              sdf=lambda m: '> <PHOREGEN_SMILES>\n%s\n\n' % m['smiles']['text'] if m['smiles'].get('smiles_ok') else '',
              compute=lambda d, opt: _smiles(d.res, screen=d.screen, kekule=d.of('kekule'), stereo=d.of('stereo') if 'stereo' in d.options else None),
              verdict=lambda m: m['smiles']['smiles_ok']),
    _Analysis('stereo', 'stereo', Stereo,
              parts=lambda x: [('t_key', x.stereo_key[0], np.uint64), ('t_status', x.status[0], np.int32), ('t_counts', x.counts[0], np.int32),
                               ('t_parity', x.atom_parity[0], np.int8), ('t_alabel', x.atom_label[0], np.int8),
                               ('t_bond', x.bond_stereo[0], np.int8), ('t_blabel', x.bond_label[0], np.int8)],
              entry=lambda x, v, at, mol: {'stereo': dict(
                  _status_entry('stereo_ok', STEREO_FAIL_MASK, STEREO_COUNTS, at.row(v['t_status']), at.row(v['t_counts'])),
                  atom_parity=at.atoms(v['t_parity']).copy(), atom_label=at.atoms(v['t_alabel']).copy(),
                  bond_stereo=at.bonds(v['t_bond']).copy(), bond_label=at.bonds(v['t_blabel']).copy(), stereo_key=int(at.row(v['t_key'])))},
              sdf=_stereo_item, read=_true_or('stereo', StereoLimits),
              compute=lambda d, opt: _stereo(d.res, screen=d.screen, kekule=d.of('kekule'), rings=d.of('rings'), keys=d.keys, limits=opt),
              verdict=lambda m: m['stereo']['stereo_ok']),
    _Analysis('fingerprints', 'fingerprint', Fingerprints, frames='fp',
              parts=lambda x: [('p_fp', x.fp[0], np.uint64), ('p_bits', x.bits[0], np.int32)],
              entry=lambda x, v, at, mol: {'fingerprint': at.row(v['p_fp']).copy(), 'fp_bits': int(at.row(v['p_bits'])), 'fp_radius': x.radius},
              sdf=_fingerprint_item, read=lambda value: None if value is False else _check_radius('sample_valid', FP_RADIUS if value is True else value),
              compute=lambda d, opt: _fingerprints(d.screen, opt)),
    # (their records live in modules of their own, which import this one)
    SimpleNamespace(keyword='substructure', key='substructure'), SimpleNamespace(keyword='hydrogens', key='hydrogens'),
]
# The analyses that joined after those nine, carried after them in this order.  (The list above is held to its nine entries, by name
# and in order, by the test of the carriers; a later analysis is one more line here instead.)
_ANALYSES_SINCE = [SimpleNamespace(keyword='properties', key='properties')]


def _blob_parts(pos_t, sc, mk, agree, handed):
    """The parts of the one blob of `assemble` as (name, final-frame tensor, numpy dtype): the screen's and the coordinates, the keys'
    (mk, None: without), the screen's agreement counts (agree) and those of every (record, holder) handed in -- the widest elements
    first, by a stable sort, so that every part stays aligned in the blob wherever its line stands.  A view has its tensor's shape."""
    parts = [('status', sc.status[0], np.int32), ('counts', sc.counts[0], np.int32), ('pos', pos_t, np.float32),
             ('compact', sc.compact[0], np.int16), ('cls', sc.cls[0], np.int8), ('valence2', sc.valence2[0], np.uint8),
             ('order', sc.order[0], np.int8)]
    if mk is not None:
        parts += [('key', mk.key[0], np.uint64), ('colour', mk.colour[0], np.uint64)]
    if agree:
        parts += [('agree', sc.agree[0], np.int32)]
    for rec, x in handed:
        parts += rec.parts(x)
    assert len({name for name, _, _ in parts}) == len(parts) and all(t.element_size() == np.dtype(dt).itemsize for _, t, dt in parts)
    return sorted(parts, key=lambda part: -np.dtype(part[2]).itemsize)


@torch.no_grad()
def assemble(results, keys=False, geometry=None, rings=None, kekule=None, features=None, smiles=None, stereo=None, fingerprints=None,
             substructure=None, screen=None, hydrogens=None, properties=None):
    """The final prediction as one dict per graph with `decode_data`'s keys and meaning -- 'element' (atomic numbers), 'atom_pos'
    (kept atoms, the tensor's own fp32 values), 'bond_index' [2, n_b] (indices among the kept atoms) and 'bond_type' [n_b] for
    a < b only, in row order -- plus 'status', 'valid', 'n_components' and 'valence' (per kept atom, halves allowed).  The screen runs
    on the device; ONE device-to-host copy brings the compact arrays over, the split by offsets is on the host.
    keys=True: every dict also has 'key' (the identity key of `molecule_keys` as an unsigned Python int) and 'atom_colour' (uint64
    per kept atom); they ride in the same copy.
    geometry=a `Geometry` of this result's final frame: every dict also has 'geom' -- 'status' (GEOM_* bits), 'geom_ok' (no bit of
    GEOM_FAIL_MASK), the eight GEOM_METRICS and the six GEOM_COUNTS by name, and 'point_dist' / 'point_atom' of the graph's points
    (an index into this dict's atoms, -1 = none) -- in the same copy; its screen is reused.
    rings=a `Rings` of this result's final frame: every dict also has 'rings' -- 'status' (RING_* bits), 'rings_ok' (no bit of
    RING_FAIL_MASK), the ten RING_COUNTS by name, 'bond_ring_size' (per entry of 'bond_type', in its order), 'atom_ring' and
    'ring_sys' (per kept atom; the system's first atom as an index into this dict's atoms, -1 = none) -- in the same copy; its screen
    is reused, and with geometry= too both must have been computed from one screen.
    kekule=a `Kekule` of this result's final frame: every dict also has 'kekule' -- 'status' (KEKULE_* bits), 'kekule_ok' (no bit of
    KEKULE_FAIL_MASK), the ten KEKULE_COUNTS by name (the count 'charge' as 'net_charge': 'charge' is per atom here), 'bond_type' (the Kekulé order per entry of the dict's 'bond_type', in its
    order; 4 stays 4 where not kekule_ok), 'hcount' and 'charge' (per kept atom), 'formula' (Hill order with the hydrogens and a
    charge suffix such as '+' / '2+') and 'mol_weight' (`formula_of`: from standard atomic weights written from memory; both computed
    on the host) -- in the same copy; its screen is reused, and it must have been computed from the screen of geometry= / rings=.
    features=a `Features` of this result's final frame: every dict also has 'features' -- 'status' (FEAT_* bits), 'features_ok' (no
    bit of FEAT_FAIL_MASK), the FEATURE_COUNTS by name, 'atom_fp' (uint8 per kept atom, bit t = FEATURE_TYPES[t]), 'atom_types' (per
    kept atom a tuple of type names), 'point_kind' of the graph's points, their 'point_dist' / 'point_atom' (the nearest atom that
    carries the point's type, an index into this dict's atoms, -1 = none) and 'point_matched' (distance < feat_cut) -- in the same copy; its screen is reused, and it must
    have been computed from the screen of the others.
    smiles=a `Smiles` of this result's final frame: every dict also has 'smiles' -- 'status' (SMILES_* bits), 'smiles_ok' (no bit of
    SMILES_FAIL_MASK), 'text' (str; '' where not ok), the eight SMILES_COUNTS by name and 'atom_rank' (per kept atom: its position in
    the text, -1 where not ok) -- in the same copy; its screen is reused, and it must have been computed from the screen of the
    others.  A `Smiles` written with stereo= also has the four SMILES_STEREO_COUNTS by name there.
    stereo=a `Stereo` of this result's final frame: every dict also has 'stereo' -- 'status' (STEREO_* bits), 'stereo_ok' (no bit of
    STEREO_FAIL_MASK), the eight STEREO_COUNTS by name, 'atom_parity' and 'atom_label' (int8 per kept atom), 'bond_stereo' and
    'bond_label' (int8 per entry of 'bond_type', in its order; all four: 0 = not stereogenic, +1 / -1, 2 = undefined) and
    'stereo_key' (an unsigned Python int) -- in the same copy; its screen is reused, and it must have been computed from the screen of
    the others.
    fingerprints=a `Fingerprints` of this result's final frame: every dict also has 'fingerprint' (np.uint64 [FP_WORDS]), 'fp_bits'
    (its set bits) and 'fp_radius' -- in the same copy; its screen is reused, and it must have been computed from the screen of the
    others.
    substructure=a `Substructure` (phoregen_amd.substructure) of this result's final frame: every dict also has 'substructure' -- per
    pattern name 'embeddings', 'anchors', 'atoms' (the atoms that lie in an embedding, indices into this dict's atoms), 'first' (the
    first embedding per query atom, None without one), 'status' (SUB_* bits) and 'status_names' -- and 'substructure_ok' (no pattern
    is SUB_OUT_OF_BOUNDS), in the same copy; its screen is reused, and it must have been computed from the screen of the others.
    screen=a `Screen` of this result's final frame: its `order` becomes 'bond_index' / 'bond_type' (so with a `screen(bonds='distance')`
    the molecules have the distance-perceived bonds); every other result handed in must have been computed from it or from one of the
    same bond source.  Every dict then also has 'bonds' (the screen's mode) and, with a `bond_agreement` screen, 'bond_agreement':
    the six BOND_AGREE_COUNTS by name.
    hydrogens=a `Hydrogens` (phoregen_amd.hydrogens) of this result's final frame: every dict also has 'hydrogens' -- 'status' (HYD_*
    bits), 'hydrogens_ok' (no bit of HYD_FAIL_MASK), the eight HYD_COUNTS by name, 'min_contact', 'h_pos' (fp32 [n_h, 3], the placed
    hydrogens in (parent, slot) order), 'h_parent' (per hydrogen an index into this dict's atoms) and 'site_shape' (per kept atom) --
    in the same copy; its screen is reused, and it must have been computed from the screen of the others.
    properties=a `Properties` (phoregen_amd.properties) of this result's final frame: every dict also has 'properties' -- 'status'
    (PROP_* bits), 'properties_ok' (no bit of PROP_FAIL_MASK), the PROPERTY_COUNTS by name, 'mol_weight', one float per table name
    (e.g. 'tpsa', 'logp', 'mr'), 'fsp3', 'violated' (the word) and 'violated_names', and per kept atom 'env' (the environment word) and
    'row' ([n, tables], the row taken per table, 255 = none) -- in the same copy; its screen is reused, and it must have been computed
    from the screen of the others."""
    handed, pos_t = _handed(locals()), results['pred'][1]              # (locals: this signature's keywords by name)
    # 1. the one screen: screen= if given, else the first holder's, else a new one; every holder must be of it
    if screen is not None and (not isinstance(screen, Screen) or screen.status.size(0) != 1 or screen.cls.size(1) != pos_t.size(-2)
                               or screen.cls.device != pos_t.device):
        raise ValueError('phoregen_amd.molecule.assemble: screen= must be a Screen of the final frame of this result')
    for rec, x in handed:
        t = getattr(x, rec.frames) if isinstance(x, rec.holder) and x.screen is not None else None
        if t is None or t.size(0) != 1 or x.screen.cls.size(1) != pos_t.size(-2) or t.device != pos_t.device:
            raise ValueError(f'phoregen_amd.molecule.assemble: {rec.keyword}= must be a {rec.holder.__name__} of the final frame of this result')
    for rec, x in handed[1:]:
        if not _same_screen(handed[0][1].screen, x.screen):
            raise ValueError(f'phoregen_amd.molecule.assemble: {handed[0][0].keyword}= and {rec.keyword}= were computed from screens of '
                             'different results')
    for rec, x in handed if screen is not None else ():
        if not _same_screen(screen, x.screen):
            raise ValueError(f'phoregen_amd.molecule.assemble: screen= and {rec.keyword}= were computed from screens of different results or '
                             f'bond sources ({screen.bonds!r}, {x.screen.bonds!r})')
    sc = screen if screen is not None else handed[0][1].screen if handed else _screen(results, 'final')
    # 2. - 4. the parts of what was handed in, widest first, in ONE copy; the views by name
    parts = _blob_parts(pos_t, sc, molecule_keys(sc) if keys else None, screen is not None and sc.agree is not None, handed)
    blob = torch.cat([t.reshape(-1).view(torch.uint8) for _, t, _ in parts]).cpu().numpy()
    cut = np.cumsum([0] + [t.numel() * t.element_size() for _, t, _ in parts])
    v = {name: blob[cut[i]:cut[i + 1]].view(dt).reshape(tuple(t.shape)) for i, (name, t, dt) in enumerate(parts)}
    # 5. the split by offsets: the base dict, then what each holder adds
    status, cls, valence2, order, compact, counts, pos = (v[k] for k in ('status', 'cls', 'valence2', 'order', 'compact', 'counts', 'pos'))
    mols, n0, h0 = [], 0, 0
    for g, n in enumerate(sc.num_atoms):
        h = n * (n - 1) // 2
        keep = cls[n0:n0 + n] >= 0
        o = order[h0:h0 + h]
        nz = np.nonzero(o)[0]
        a, b = _pairs(n)
        at = _MolView(g, n0, n, keep, h0, h, nz, compact[n0:n0 + n].astype(np.int64))
        mol = {'element': [ATOM_TYPES[c] for c in at.atoms(cls).tolist()],
               'atom_pos': torch.from_numpy(at.atoms(pos)),
               'bond_index': torch.from_numpy(np.stack([at.cmp_g[a[nz]], at.cmp_g[b[nz]]])),
               'bond_type': torch.from_numpy(o[nz].astype(np.int64)),
               'status': int(status[g]), 'valid': (int(status[g]) & FAIL_MASK) == 0, 'n_components': int(counts[g, 2]),
               'valence': at.atoms(valence2).astype(np.float64) / 2.0}
        if screen is not None:
            mol['bonds'] = sc.bonds
            if sc.agree is not None:
                mol['bond_agreement'] = {k: int(x) for k, x in zip(BOND_AGREE_COUNTS, at.row(v['agree']))}
        if keys:
            mol['key'], mol['atom_colour'] = int(at.row(v['key'])), at.atoms(v['colour']).copy()
        for rec, x in handed:
            mol.update(rec.entry(x, v, at, mol))
        mols.append(mol)
        n0, h0 = n0 + n, h0 + h
    return mols


# ---- V2000 mol blocks (CTfile format) ---------------------------------------------------------------------------------------
def mol_block(mol, name=''):
    """One V2000 mol block of an assembled molecule: three header lines (name, program line with the '3D' flag, empty comment),
    the counts line, one line per atom and per bond (type 4 = aromatic), 'M  END'.
    A molecule that carries 'kekule' (assemble(kekule=)) with 'kekule_ok' is written in Kekulé form: bond types 1 / 2 / 3 from
    kekule['bond_type'], a charged atom's charge in the atom line's `ccc` field (3 = +1, 2 = +2, 1 = +3, 5 = -1, 6 = -2, 7 = -3) and in
    'M  CHG' lines of at most eight entries before 'M  END'.  Hydrogens stay implicit.  Without 'kekule', or with a failed one, the
    block is as it always was.
    A molecule that also carries 'hydrogens' (assemble(hydrogens=)) with 'hydrogens_ok' -- and 'kekule' with 'kekule_ok' -- is written
    as an all-atom block: after the heavy atoms one 'H' line per placed hydrogen in (parent, slot) order, after the heavy bonds one
    type-1 bond line per hydrogen from its parent.  In every other case the block is byte for byte what it is without 'hydrogens'."""
    elements, pos = mol['element'], np.asarray(mol['atom_pos'], dtype=np.float64).reshape(-1, 3)
    bi, bt = np.asarray(mol['bond_index']).reshape(2, -1), np.asarray(mol['bond_type']).reshape(-1)
    kek = mol.get('kekule')
    kek = kek if kek is not None and kek.get('kekule_ok') else None
    charge = [0] * len(elements)
    if kek is not None:
        bt, charge = np.asarray(kek['bond_type']).reshape(-1), [int(q) for q in np.asarray(kek['charge']).reshape(-1).tolist()]
        if bt.size != bi.shape[1] or len(charge) != len(elements) or any(abs(q) > 3 for q in charge):
            raise ValueError(f"mol_block: 'kekule' has {bt.size} bond types and {len(charge)} charges for {bi.shape[1]} bonds and "
                             f'{len(elements)} atoms (charges within -3 .. 3)')
    hyd = mol.get('hydrogens') if kek is not None else None
    hyd = hyd if hyd is not None and hyd.get('hydrogens_ok') else None
    h_pos, h_parent = np.zeros((0, 3)), []
    if hyd is not None:
        h_pos, h_parent = np.asarray(hyd['h_pos'], dtype=np.float64).reshape(-1, 3), np.asarray(hyd['h_parent']).reshape(-1).tolist()
        if len(h_parent) != len(h_pos) or any(not 0 <= a < len(elements) for a in h_parent):
            raise ValueError(f"mol_block: 'hydrogens' has {len(h_pos)} positions and {len(h_parent)} parents among {len(elements)} atoms")
    n_all, n_bonds = len(elements) + len(h_parent), bt.size + len(h_parent)
    if n_all > 999 or n_bonds > 999:
        raise ValueError(f'mol_block: {n_all} atoms / {n_bonds} bonds do not fit the 3-digit counts of a V2000 block')
    if not (np.isfinite(pos).all() and np.isfinite(h_pos).all()):
        raise ValueError('mol_block: non-finite coordinates')
    lines = [str(name).split('\n')[0], '  PhoreGen' + ' ' * 10 + '3D', '',
             '%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (n_all, n_bonds)]
    for z, (x, y, zc), q in zip(elements, pos.tolist(), charge):
        lines.append('%10.4f%10.4f%10.4f %-3s 0%3d  0  0  0  0  0  0  0  0  0  0' % (x, y, zc, ELEMENT_SYMBOL[int(z)], (4 - q) if q else 0))
    for x, y, zc in h_pos.tolist():
        lines.append('%10.4f%10.4f%10.4f %-3s 0%3d  0  0  0  0  0  0  0  0  0  0' % (x, y, zc, 'H', 0))
    for (a, b), t in zip(bi.T.tolist(), bt.tolist()):
        lines.append('%3d%3d%3d  0' % (a + 1, b + 1, t))
    for k, a in enumerate(h_parent):
        lines.append('%3d%3d%3d  0' % (a + 1, len(elements) + k + 1, 1))
    charged = [(i + 1, q) for i, q in enumerate(charge) if q]
    for k in range(0, len(charged), 8):
        lines.append('M  CHG%3d' % len(charged[k:k + 8]) + ''.join(' %3d %3d' % e for e in charged[k:k + 8]))
    lines.append('M  END')
    return '\n'.join(lines) + '\n'


def _bonds_item(m):
    """The PHOREGEN_BONDS data item of a molecule that carries 'bonds' (`assemble(screen=)`)."""
    ag = m.get('bond_agreement')
    return '> <PHOREGEN_BONDS>\nmode %s\n' % m['bonds'] + ('' if ag is None else ''.join('%s %d\n' % (k, ag[k]) for k in BOND_AGREE_COUNTS)) + '\n'


def write_sdf(path, mols, names=None):
    """An SDF file: one mol block per molecule, each closed by a '$$$$' line.  A molecule that carries 'key' (assemble(keys=True))
    gets one data item `> <PHOREGEN_KEY>` with the key as 16 hex digits between its block and the '$$$$'.  A molecule that carries
    'geom' (assemble(geometry=)) gets `> <PHOREGEN_GEOM>`: one line with the status as hex, then one 'name value' line per metric
    (GEOM_METRICS without the reserved one) with four decimals.  A molecule that carries 'rings' (assemble(rings=)) gets
    `> <PHOREGEN_RINGS>`: one line with the status as hex, then one 'name value' line per count (RING_COUNTS).  A molecule that
    carries 'kekule' (assemble(kekule=)) is written in Kekulé form if that is ok (`mol_block`) and gets `> <PHOREGEN_KEKULE>`: the
    status as hex, 'formula', 'mol_weight' with three decimals, then one 'name value' line per count (KEKULE_COUNTS).  A molecule that
    carries 'features' (assemble(features=)) gets `> <PHOREGEN_FEATURES>`: the status as hex, one 'name value' line per count
    (FEATURE_COUNTS), then one line per typed point: its type, the matched atom (1-based; '-' if no atom of the type lies within the
    cutoff) and the distance to the nearest atom of the type with four decimals ('inf' without one).  A molecule that carries 'smiles'
    (assemble(smiles=)) with 'smiles_ok' gets `> <PHOREGEN_SMILES>` with the text on one line; a failed one gets no item.  A molecule
    that carries 'stereo' (assemble(stereo=)) gets `> <PHOREGEN_STEREO>`: the status as hex, 'stereo_key' as 16 hex digits, one 'name
    value' line per count (STEREO_COUNTS), then one line 'centre atom parity label' per stereogenic centre (atom 1-based) and one line
    'bond atom atom stereo label' per stereogenic double bond, values as '+', '-' or '?' (undefined).  The mol block itself does not
    change: its 3D coordinates carry the stereo.  A molecule that carries 'fingerprint' (assemble(fingerprints=)) gets
    `> <PHOREGEN_FINGERPRINT>`: one line of 512 hex digits, word 0 first, each word as 16 digits, then 'radius R'.  A molecule that
    carries 'substructure' (assemble(substructure=)) gets `> <PHOREGEN_SUBSTRUCTURE>`: one line per pattern with its name, embeddings,
    anchors, the status as hex, the atoms that lie in an embedding and the first embedding (1-based, comma-separated, '-' if empty;
    `phoregen_amd.substructure.parse_sdf_item` reads it back).  A molecule that carries 'bonds' (assemble(screen=)) gets `> <PHOREGEN_BONDS>`:
    'mode predicted' or 'mode distance', then, if it also carries 'bond_agreement', one 'name value' line per count
    (BOND_AGREE_COUNTS).  A molecule that carries 'hydrogens' (assemble(hydrogens=)) is written as an all-atom block if that and its
    Kekulé form are ok (`mol_block`) and gets `> <PHOREGEN_HYDROGENS>`: the status as hex, one 'name value' line per count (HYD_COUNTS of
    phoregen_amd.hydrogens) and 'min_contact' with four decimals ('inf' without a pair).  A molecule that carries 'properties'
    (assemble(properties=)) gets `> <PHOREGEN_PROPERTIES>`: the status as hex, 'mol_weight' with three decimals, one line per table
    name and 'fsp3' with four, one 'name value' line per count (PROPERTY_COUNTS of phoregen_amd.properties) and the names of the
    violated quantities ('-' for none).  A molecule without one gets no such item: the text is as it always was."""
    names = names if names is not None else [''] * len(mols)
    if len(names) != len(mols):
        raise ValueError(f'write_sdf: {len(mols)} molecules, {len(names)} names')
    with open(path, 'w') as fh:
        for m, nm in zip(mols, names):
            fh.write(mol_block(m, nm))
            fh.write((_bonds_item(m) if 'bonds' in m else '') + ('> <PHOREGEN_KEY>\n%016x\n\n' % (int(m['key']) & _M64) if 'key' in m else ''))
            fh.write(''.join(rec.sdf(m) for rec in _carried(lambda a: a.key in m)))
            fh.write('$$$$\n')


# ---- identity: exact comparison and grouping of assembled molecules ---------------------------------------------------------

def _mol_graph(m, stereo=False):
    """Adjacency {neighbour: order} per atom, the atoms' exact local signatures and the colours handed in (all equal if absent).
    stereo: a bond's label is its order and its 'bond_label', an atom's own signature has its 'atom_label'."""
    n = len(m['element'])
    bi, bt = np.asarray(m['bond_index']).reshape(2, -1), np.asarray(m['bond_type']).reshape(-1)
    al, bl = [0] * n, [0] * bt.size
    if stereo:
        if 'stereo' not in m:
            raise ValueError("same_molecule: stereo=True needs molecules that carry 'stereo' (assemble(stereo=))")
        al, bl = np.asarray(m['stereo']['atom_label']).reshape(-1).tolist(), np.asarray(m['stereo']['bond_label']).reshape(-1).tolist()
        if len(al) != n or len(bl) != bt.size:
            raise ValueError(f"same_molecule: {n} atoms and {bt.size} bonds, 'stereo' has {len(al)} and {len(bl)} labels")
    adj = [{} for _ in range(n)]
    for a, b, t, l in zip(bi[0].tolist(), bi[1].tolist(), bt.tolist(), bl):
        adj[a][b] = adj[b][a] = int(t) | (int(l) & 0xff) << 8
    own = [(int(z), int(l), tuple(sorted(nb.values()))) for z, l, nb in zip(m['element'], al, adj)]
    col = m.get('atom_colour')
    col = [0] * n if col is None else [int(c) & _M64 for c in np.asarray(col).reshape(-1).tolist()]
    if len(col) != n:
        raise ValueError(f"same_molecule: {n} atoms, {len(col)} entries in 'atom_colour'")
    # what an atom sees of itself and of its neighbours is the same in any numbering, so it may always restrict the candidates
    sig = [(own[i], tuple(sorted((t, own[j]) for j, t in adj[i].items())), col[i]) for i in range(n)]
    return adj, sig


def _components(adj):
    """Connected components as lists of atoms in breadth-first order: every atom but the first has an earlier neighbour."""
    seen, comps = [False] * len(adj), []
    for s in range(len(adj)):
        if seen[s]:
            continue
        seen[s], comp = True, [s]
        for u in comp:                                                 # (grows while it is walked)
            for v in sorted(adj[u]):
                if not seen[v]:
                    seen[v] = True
                    comp.append(v)
        comps.append(comp)
    return comps


def _component_matches(c1, adj1, sig1, c2, adj2, sig2):
    """Is there a bijection of the atoms of c1 onto those of c2 that keeps signatures and bond orders?  Backtracking in the
    breadth-first order of c1: an atom's image is looked for among the neighbours of its first mapped neighbour's image."""
    if len(c1) != len(c2) or sorted(sig1[i] for i in c1) != sorted(sig2[j] for j in c2):
        return False
    place = {a: k for k, a in enumerate(c1)}
    earlier = [[(b, t) for b, t in adj1[a].items() if place[b] < k] for k, a in enumerate(c1)]
    image, used = {}, set()

    def extend(k):
        if k == len(c1):
            return True
        a = c1[k]
        cands = adj2[image[earlier[k][0][0]]] if earlier[k] else c2
        for x in cands:
            if x in used or sig2[x] != sig1[a] or any(adj2[x].get(image[b]) != t for b, t in earlier[k]):
                continue
            # (bonds of x that a lacks need no check: signatures hold the degree, so both components have as many bonds, and once
            # every atom is placed every bond of c1 has its own bond of c2)
            image[a] = x
            used.add(x)
            if extend(k + 1):
                return True
            del image[a]
            used.discard(x)
        return False

    return extend(0)


def same_molecule(m1, m2, stereo=False):
    """Exact: do two assembled molecules have the same atoms and bonds up to a renumbering of the atoms (elements and bond orders as
    labels, 4 = aromatic its own label; coordinates play no part)?  'atom_colour', where both carry it, only narrows the search: with
    any colours, all equal included, the answer is the same, as long as equal molecules were coloured by the same rule.
    stereo=True (both must carry 'stereo', assemble(stereo=)): the renumbering must also keep every 'atom_label' and 'bond_label', so
    two enantiomers, or a cis and a trans isomer, differ.  The labels are relative to the colours: this is exact as far as atoms
    with equal colours are equivalent, and an undefined element (2) only equals an undefined one."""
    if len(m1['element']) != len(m2['element']) or np.asarray(m1['bond_type']).size != np.asarray(m2['bond_type']).size:
        return False
    if ('atom_colour' in m1) != ('atom_colour' in m2):                  # colours of one side only say nothing: drop them
        m1, m2 = ({k: v for k, v in m.items() if k != 'atom_colour'} for m in (m1, m2))
    (adj1, sig1), (adj2, sig2) = _mol_graph(m1, stereo), _mol_graph(m2, stereo)
    if sorted(sig1) != sorted(sig2):
        return False
    comps1, comps2 = _components(adj1), _components(adj2)
    if len(comps1) != len(comps2):
        return False
    # components pair off greedily: being the same component is an equivalence, so any partner of that kind will do
    free = list(comps2)
    for c1 in comps1:
        hit = next((k for k, c2 in enumerate(free) if _component_matches(c1, adj1, sig1, c2, adj2, sig2)), None)
        if hit is None:
            return False
        free.pop(hit)
    return True


def unique_molecules(mols, stereo=False):
    """The partition of assembled molecules into classes of `same_molecule`: (representatives, class_of) with the first member of
    every class as its representative, in order of appearance, and class_of[i] the index into `representatives` of mols[i].
    If every molecule carries 'key', a molecule is only compared inside its key's group (equal molecules have equal keys); the
    answer is exact either way.  stereo=True: the classes of `same_molecule(stereo=True)`, grouped by 'stereo_key' -- stereoisomers
    are separate molecules; every molecule must carry 'stereo'."""
    reps, class_of, by_key = [], [], {}
    keyed = all('key' in m for m in mols) and not stereo
    for m in mols:
        group = by_key.setdefault(int(m['stereo']['stereo_key']) & _M64 if stereo else int(m['key']) & _M64 if keyed else None, [])
        hit = next((r for r in group if same_molecule(reps[r], m, stereo)), None)
        if hit is None:
            hit = len(reps)
            reps.append(m)
            group.append(hit)
        class_of.append(hit)
    return reps, class_of


@torch.no_grad()
def duplicate_groups(keys):
    """Key-level census of a key vector on its own device, no host loop: (first, counts, group) with first[k] the index of the first
    occurrence of the k-th distinct key (ascending, so in order of appearance), counts[k] how often it occurs and group[i] the k of
    keys[i].  KEY-LEVEL ONLY: molecules with different keys differ, molecules with one key are very likely, not certainly, the same --
    copy the representatives `keys[first]` points at and let `unique_molecules` confirm where that matters.  Handed a `Stereo`'s
    `stereo_key` instead of a `MolKeys`' `key`, the census counts stereoisomers separately."""
    keys = keys.reshape(-1)
    n, dev = keys.numel(), keys.device
    srt, perm = torch.sort(keys, stable=True)                          # stable: the first occurrence leads its run
    new = torch.ones(n, dtype=torch.bool, device=dev)
    new[1:] = srt[1:] != srt[:-1]
    starts = new.nonzero().reshape(-1)
    counts = torch.diff(starts, append=torch.tensor([n], device=dev))
    first, by_first = perm[starts].sort()
    rank = torch.empty_like(by_first)
    rank[by_first] = torch.arange(by_first.numel(), device=dev)
    group = torch.empty(n, dtype=torch.long, device=dev)
    group[perm] = rank[new.cumsum(0) - 1]
    return first, counts[by_first], group


# ---- the top-up loop of sample_all.py:79-84,172 ------------------------------------------------------------------------------
class _Draw:
    """One draw of `sample_valid`, and the one place where its analyses are computed: its screen, its keys and the holder of every
    analysis (`of`), each on first demand and at most once.  An analysis is computed (its record's `compute`, which takes what it
    needs from the draw again) with what the user gave for its keyword -- `options`, {keyword: what the record's `read` made of the
    argument} -- else with the defaults."""

    def __init__(self, res, data, model, options, add_edge='predicted', margins=None, agreement=False):
        self.res, self.data, self.model, self.options, self._held = res, data, model, options, {}
        self.add_edge, self.margins, self.agreement = add_edge, margins or BondMargins(), agreement

    def of(self, keyword):
        if keyword not in self._held:
            rec, = _carried(lambda a: a.keyword == keyword)
            self._held[keyword] = rec.compute(self, self.options[keyword] if keyword in self.options else rec.read(True))
        return self._held[keyword]

    @cached_property
    def screen(self):
        """The draw's screen in its bond mode; with `agreement` it carries the counts of `bond_agreement` in either mode."""
        if self.add_edge == 'predicted':
            sc = _screen(self.res, 'final')
            return replace(sc, agree=bond_agreement(self.res, 'final', self.margins).agree) if self.agreement else sc
        if self.agreement:
            return bond_agreement(self.res, 'final', self.margins)
        return _screen(self.res, 'final', bonds=self.add_edge, margins=self.margins)

    @cached_property
    def keys(self):
        return molecule_keys(self.screen)


def _identity(m):
    """`sample_valid(unique=True)`: (the key a molecule is looked up by, `same_molecule`'s stereo=), by whether it carries 'stereo'."""
    return (m['stereo']['stereo_key'], True) if 'stereo' in m else (m['key'], False)


def sample_valid(model, data, num_samples, batch_size=30, max_failed_factor=3, device='cuda', unique=False, geometry=None,
                 rings=None, kekule=None, features=None, smiles=None, stereo=None, fingerprints=None, substructure=None,
                 add_edge='predicted', bond_margins=None, bond_agreement=False, hydrogens=None, properties=None, **sample_kwargs):
    """Sample until `num_samples` molecules have passed the screen, giving up once more than `max_failed_factor * num_samples` have
    failed (checked before every draw, as the reference does).  Every draw asks for min(batch_size, what is still missing) graphs,
    so never more than `num_samples` are finished.  `sample_kwargs` (fragment=, pos_guidance_opt=, rng=, seed=, ...) go to
    `model.sample`; a fixed seed= repeats the same draw in every call of the same size, so leave it unset (a fresh key per call, drawn
    from torch's default generator) unless that is meant.  Returns {'finished': [...], 'failed': [...], 'n_calls': int} with `assemble`'s dicts.
    unique=True: a valid molecule is finished only if it is not `same_molecule` to one already finished (looked up by key, confirmed
    exactly); a repeat goes to the additional list 'duplicates', counts neither as finished nor as failed, and the loop also gives up
    once more than `max_failed_factor * num_samples` repeats have been seen.  The molecules then carry 'key' and 'atom_colour'.
    geometry=(point_pos, point_is_ex, limits), or True to take the pharmacophore of `data` (`geometry_for`, default limits): a valid
    molecule is finished only if it is also 'geom_ok'; one that is not goes to 'failed'.  The molecules then carry 'geom'.
    rings=a `RingLimits`, or True for the default limits: a valid molecule is finished only if it is also 'rings_ok'; one that is not
    goes to 'failed'.  The molecules then carry 'rings'.
    kekule=a `KekuleOptions`, or True for the default options: a valid molecule is finished only if it is also 'kekule_ok' (it has a
    Kekulé structure); one that is not goes to 'failed'.  The molecules then carry 'kekule'.
    features=(point_pos, point_kind, limits), or True to take the pharmacophore of `data` (`features_for`, default limits): a valid
    molecule is finished only if it is also 'features_ok'; one that is not goes to 'failed'.  The molecules then carry 'features'.
    The typing needs the Kekulé form and the rings of the draw: they are computed (with kekule= / rings= if given, else with the
    defaults) and carried, and filtered on, only if asked for by their own arguments.
    smiles=True: a valid molecule is finished only if it is also 'smiles_ok' -- it has a Kekulé structure and its text was written;
    one that is not goes to 'failed'.  The molecules then carry 'smiles'.  The text needs the Kekulé form of the draw: it is computed
    (with kekule= if given, else with the default options) and carried, as 'kekule', only if asked for by its own argument.
    stereo=a `StereoLimits`, or True for the default limits: a valid molecule is finished only if it is also 'stereo_ok'; one that is
    not goes to 'failed'.  The molecules then carry 'stereo'; with smiles=True the text is isomeric; with unique=True stereoisomers
    count as different molecules (looked up by 'stereo_key', confirmed by `same_molecule(stereo=True)`).  The Kekulé form and the
    rings it needs are computed and carried as for features=.
    fingerprints=True for the default radius, or a radius 0 .. FP_MAX_RADIUS: the molecules then carry 'fingerprint', 'fp_bits' and
    'fp_radius'; nothing is filtered on them.
    substructure=a list of `Pattern`s (phoregen_amd.substructure), or (patterns, max_steps): a valid molecule is finished only if it is
    also 'substructure_ok' -- for every pattern `anchors` lies within the pattern's min / max, and no bounded pattern was truncated;
    one that is not goes to 'failed'.  The molecules then carry 'substructure'.  The rings and the Kekulé form it needs are computed
    and carried as for features=.
    add_edge='predicted' (the reference driver's `--add_edge` spelling): the bonds are the argmax of the edge scores.  'distance': they
    are perceived from the sampled coordinates (`screen(bonds='distance')`, with bond_margins= a `BondMargins` or the defaults);
    validity and every analysis above then run on that screen, and the molecules carry 'bonds'.  'openbabel' is not supported.
    bond_agreement=True: the molecules also carry 'bonds' and 'bond_agreement' (the six BOND_AGREE_COUNTS of the predicted against the
    distance bonds, `bond_agreement`), in either mode; nothing is filtered on them.
    hydrogens=a `HydrogenOptions` (phoregen_amd.hydrogens), or True for the default options: a valid molecule is finished only if it is
    also 'hydrogens_ok' -- it has a Kekulé structure, finite coordinates and no more contacts than the options allow; one that is not
    goes to 'failed'.  The molecules then carry 'hydrogens' and, since an all-atom block needs it, the Kekulé form of the draw as
    'kekule' (computed with kekule= if given, else with the default options), so `write_sdf` writes all-atom blocks.
    properties=a `PropertyLimits` (phoregen_amd.properties) for the default tables, (tables, limits), or True for the default tables
    without a limit: a valid molecule is finished only if it is also 'properties_ok' -- it has a Kekulé structure and no more
    violated limits than the limits allow, e.g. properties=PropertyLimits.lipinski(); one that is not goes to 'failed', so the loop
    tops up until `num_samples` pass.  The molecules then carry 'properties'.  The Kekulé form and the rings it needs are computed and
    carried as for features=.
    All of these share one screen per draw."""
    args = locals()                                                    # (this signature's keywords by name, for the records' readers)
    if add_edge not in BOND_MODES:
        raise ValueError(f'phoregen_amd.molecule.sample_valid: add_edge must be one of {BOND_MODES}, not {add_edge!r}')
    if bond_margins is not None and not isinstance(bond_margins, BondMargins):
        raise ValueError(f'phoregen_amd.molecule.sample_valid: bond_margins= must be a BondMargins, not {bond_margins!r}')
    options = {rec.keyword: opt for rec, value in _handed(args) if (opt := rec.read(value)) is not None}      # (a reader's None: not asked for)
    carry = set(options).union(*(rec.also for rec in _carried(lambda a: a.keyword in options)))
    carried = _carried(lambda a: a.keyword in carry)                            # carried, and filtered on where there is a verdict
    finished, failed, duplicates, n_calls = [], [], [], 0
    by_key = {}                                                        # key -> finished molecules that have it
    while len(finished) < num_samples:
        if len(failed) > max_failed_factor * num_samples or len(duplicates) > max_failed_factor * num_samples:
            break
        n = min(batch_size, num_samples - len(finished))
        res = model.sample(data, n, device, return_traj=False, **sample_kwargs)
        n_calls += 1
        draw = _Draw(res, data, model, options, add_edge, bond_margins, bool(bond_agreement))
        held = {rec.keyword: draw.of(rec.keyword) for rec in carried}
        if add_edge != 'predicted' or bond_agreement:
            held['screen'] = draw.screen
        for m in assemble(res, keys=unique, **held):
            if not m['valid'] or not all(rec.verdict(m) for rec in carried if rec.verdict is not None):
                failed.append(m)
                continue
            key, labels = _identity(m) if unique else (None, False)
            if unique and any(same_molecule(m, other, labels) for other in by_key.setdefault(key, [])):
                duplicates.append(m)
            else:
                finished.append(m)
                if unique:
                    by_key[key].append(m)
    out = {'finished': finished, 'failed': failed, 'n_calls': n_calls}
    if unique:
        out['duplicates'] = duplicates
    return out
