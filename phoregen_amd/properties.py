"""Property descriptors and drug-likeness limits of decoded molecules on the device (csrc/mol_props.hip, csrc/props_core.h; DESIGN.md
2.9 "Properties"): molecular weight, additive atom-contribution sums (polar surface area, logP, molar refractivity), the Lipinski and
Veber counts, Fsp3, and a verdict against limits -- so that "n drug-like molecules for this pharmacophore" needs no host toolkit.

`properties` computes, for every decoded (frame, graph) in one launch, an *environment word* per kept atom -- 30 bits that say what the
atom is and what surrounds it (`ENV_FIELDS`, `env_fields`): element, hydrogens, charge, degree, aromatic, double and triple bonds, ring
membership, and counts and flags of its neighbours -- from the screen, the Kekulé form and the rings, without coordinates.  A
`PropertyTable` is data: rows `(mask, value, atom, per_h)`; an atom takes the first row with `(env & mask) == value` and adds
`atom + hcount * per_h` (units of 1e-4) to the graph's sum for that table; an atom without a row adds 0 and is counted as untyped.
The counts (`PROPERTY_COUNTS`) and the weight come from the same words.  `PropertyLimits` turns them into a verdict
(`PropertyLimits.lipinski()`, `PropertyLimits.veber()`).  Everything is integer work: results are exact and do not depend on the
numbering of the atoms.  `molecule.assemble(properties=)`, `molecule.sample_valid(properties=)` and `molecule.write_sdf` carry them.

The shipped tables (`TPSA`, `TPSA_SP`, `LOGP`, `MR`; this module holds their only copy) are Ertl's polar-surface fragment
contributions and Wildman-Crippen-style atom contributions, as far as the environment word can tell the published types apart, with
every hydrogen contribution carried as the parent row's `per_h`.  CAVEAT, as for `molecule.MAX_VALENCE`: the values are written from
memory, not checked against RDKit -- neither RDKit nor the papers were at hand.  Where the word merges several published types one
value was picked; the merges are listed at the tables.  A user with the papers replaces a table by passing their own `PropertyTable`.

What this is not: no QED and no synthetic-accessibility score -- QED's desirability-function parameters and SA's fragment table
cannot be written down reliably here; no count of aromatic rings, which would need a ring list; and TPSA, logP and MR are this
project's typing of published schemes, not RDKit's numbers.  `molecule.KEKULE_COUNTS`' hbd / hba, `molecule.RING_COUNTS`' rotatable
(no amide or terminal exceptions) and the host-side `mol_weight` of `assemble(kekule=)` keep their own definitions."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import hip
from . import molecule as M
from .utils.sample_utils import ATOM_TYPES

MAX_ROWS, MAX_TABLES = hip.PG_PROP_MAX_ROWS, hip.PG_PROP_MAX_TABLES
PROP_NO_KEKULE = 1               # the graph's Kekulé status has KEKULE_FAILED: counts, sums and weight are 0, every word is -1
PROP_LIMITS = 2                  # more violated quantities than max_violations
PROP_UNTYPED = 4                 # informational: an atom without a row in one of the tables
PROP_FAIL_MASK = PROP_NO_KEKULE | PROP_LIMITS
PROP_NAMES = {PROP_NO_KEKULE: 'NO_KEKULE', PROP_LIMITS: 'LIMITS', PROP_UNTYPED: 'UNTYPED'}
PROPERTY_COUNTS = ('heavy_atoms', 'hydrogens', 'carbons', 'sp3_carbons', 'heteroatoms', 'halogens', 'nhoh', 'no_count', 'rotatable',
                   'amide_bonds', 'aromatic_atoms', 'ring_atoms', 'net_charge', 'untyped', 'violations', 'reserved')
# the limited quantities, in the order of the bits of `violated`; after them the sums of tables 0..3
LIMITED = ('mol_weight', 'heavy_atoms', 'nhoh', 'no_count', 'rotatable')
SUM_UNIT, WEIGHT_UNIT = 10 ** 4, 10 ** 3     # a contribution is an integer number of 1e-4, a weight of 1e-3
VALUE_BOUND = 1 << 20                        # |atom|, |per_h| of a row stay below this: 128 atoms of 15 hydrogens cannot leave int32
_INT_MIN, _INT_MAX = -2 ** 31, 2 ** 31 - 1

# field -> (shift, width) of the environment word (the PG_PROP_ENV_* macros); bits 30 and 31 are 0
ENV_FIELDS = {'el': (hip.PG_PROP_ENV_EL, 4), 'h': (hip.PG_PROP_ENV_H, 3), 'q': (hip.PG_PROP_ENV_Q, 1), 'deg': (hip.PG_PROP_ENV_DEG, 3),
              'arom': (hip.PG_PROP_ENV_AROM, 1), 'n_dbl': (hip.PG_PROP_ENV_N_DBL, 2), 'triple': (hip.PG_PROP_ENV_TRIPLE, 1),
              'ring': (hip.PG_PROP_ENV_RING, 1), 'ring3': (hip.PG_PROP_ENV_RING3, 1), 'nb_het': (hip.PG_PROP_ENV_NB_HET, 3),
              'nb_arom': (hip.PG_PROP_ENV_NB_AROM, 2), 'dbl_o': (hip.PG_PROP_ENV_DBL_O, 1), 'dbl_het': (hip.PG_PROP_ENV_DBL_HET, 1),
              'nb_dbl_het': (hip.PG_PROP_ENV_NB_DBL_HET, 1), 'nb_hal': (hip.PG_PROP_ENV_NB_HAL, 2), 'nb_no': (hip.PG_PROP_ENV_NB_NO, 3)}


def env_fields(word):
    """An environment word as {field: value} in the order of `ENV_FIELDS`; None for -1 (a dropped atom, or no Kekulé structure)."""
    word = int(word)
    if word < 0:
        return None
    return {k: (word >> s) & ((1 << w) - 1) for k, (s, w) in ENV_FIELDS.items()}


def table_row(atom, per_h=0.0, **fields):
    """One row (mask, value, atom, per_h) of a `PropertyTable`: it matches the words whose `fields` (names of `ENV_FIELDS`) have
    exactly the given values; `atom` and `per_h` are the contributions of the atom and of each of its hydrogens, as numbers that are
    rounded to 1e-4.  No field: the row matches every atom."""
    mask = value = 0
    for k, x in fields.items():
        if k not in ENV_FIELDS:
            raise ValueError(f'phoregen_amd.properties.table_row: {k!r} is no field of the environment word {tuple(ENV_FIELDS)}')
        s, w = ENV_FIELDS[k]
        x = M._check_int('phoregen_amd.properties.table_row', k, x, 0, (1 << w) - 1)
        mask, value = mask | ((1 << w) - 1) << s, value | x << s
    return mask, value, round(atom * SUM_UNIT), round(per_h * SUM_UNIT)


@dataclass(frozen=True)
class PropertyTable:
    """A named contribution table: up to MAX_ROWS rows (mask, value, atom, per_h) of integers -- two int32 for the match, two
    contributions in units of 1e-4 with |.| < 2 ** 20 (`table_row` makes one from field names and numbers).  An atom takes the FIRST
    row with (env & mask) == value.  The name keys the sum in `Properties.value`, in `PropertyLimits.sums` and in a molecule's dict."""
    name: str
    rows: tuple = ()

    def __post_init__(self):
        who = 'phoregen_amd.properties.PropertyTable'
        if not isinstance(self.name, str) or not self.name or self.name != self.name.strip() or len(self.name.split()) != 1:
            raise ValueError(f'{who}: name must be one word, not {self.name!r}')
        if self.name in LIMITED or self.name in PROPERTY_COUNTS or self.name in ('status', 'properties_ok', 'fsp3', 'violated', 'violated_names', 'env', 'row'):
            raise ValueError(f'{who}: the name {self.name!r} is taken by an entry of a molecule\'s properties')
        rows = tuple(tuple(r) for r in self.rows)
        if len(rows) > MAX_ROWS:
            raise ValueError(f'{who} {self.name!r}: {len(rows)} rows, a table holds at most MAX_ROWS = {MAX_ROWS}')
        out = []
        for i, r in enumerate(rows):
            if len(r) != 4:
                raise ValueError(f'{who} {self.name!r}: row {i} must be (mask, value, atom, per_h), not {r!r}')
            mask = M._check_int(who, f'{self.name!r} row {i} mask', r[0], _INT_MIN, _INT_MAX)
            value = M._check_int(who, f'{self.name!r} row {i} value', r[1], _INT_MIN, _INT_MAX)
            atom = M._check_int(who, f'{self.name!r} row {i} atom', r[2], 1 - VALUE_BOUND, VALUE_BOUND - 1)
            per_h = M._check_int(who, f'{self.name!r} row {i} per_h', r[3], 1 - VALUE_BOUND, VALUE_BOUND - 1)
            out.append((mask, value, atom, per_h))
        object.__setattr__(self, 'rows', tuple(out))


# ---- the shipped tables --------------------------------------------------------------------------------------------------------------
# CAVEAT: every number below is written from memory, not checked against RDKit or against the papers (Ertl, Rohde, Selzer, J. Med.
# Chem. 2000; Wildman, Crippen, J. Chem. Inf. Comput. Sci. 1999).  These are the tables' only copies: the kernel and the tests'
# restatement are handed them.
_B, _C, _N, _O, _F, _SI, _P, _S, _CL, _BR, _I = range(11)


def _rows(spec, column):
    return tuple(table_row(v[column][0], v[column][1], **f) for f, v in spec)


def _one(f, atom, per_h=0.0):                                         # a row spec of a table with one value column
    return f, ((atom, per_h),)


# Ertl's polar surface contributions of N and O (Angstrom^2); a hydrogen's share is part of the fragment's value, so per_h = 0.
# Merged: the anion rows are left out (the Kekulé form has no negative charge); [n](=*)(:*):* is every neutral aromatic N of degree
# 3 with a non-aromatic double bond; an N or O that fits no fragment takes its element's last row (a choice, not Ertl's); every other
# element adds 0 through the last row, so no atom is untyped.
_TPSA = [
    _one(dict(el=_N, arom=0, q=0, h=0, triple=1, n_dbl=0), 23.79),    # [N]#*
    _one(dict(el=_N, arom=0, q=0, h=0, triple=1), 13.60),             # [N](=*)#*
    _one(dict(el=_N, arom=0, q=0, h=0, n_dbl=0, ring3=1, deg=3), 3.01),   # [N]1(-*)-*-*-1
    _one(dict(el=_N, arom=0, q=0, h=0, n_dbl=0), 3.24),               # [N](-*)(-*)-*
    _one(dict(el=_N, arom=0, q=0, h=0, n_dbl=1), 12.36),              # [N](-*)=*
    _one(dict(el=_N, arom=0, q=0, h=0), 11.68),                       # [N](-*)(=*)=*
    _one(dict(el=_N, arom=0, q=0, h=1, n_dbl=0, ring3=1), 21.94),     # [NH]1-*-*-1
    _one(dict(el=_N, arom=0, q=0, h=1, n_dbl=0), 12.03),              # [NH](-*)-*
    _one(dict(el=_N, arom=0, q=0, h=1), 23.85),                       # [NH]=*
    _one(dict(el=_N, arom=0, q=0, h=2), 26.02),                       # [NH2]-*
    _one(dict(el=_N, arom=0, q=1, h=0, triple=1), 4.36),              # [N+](-*)#*
    _one(dict(el=_N, arom=0, q=1, h=0, n_dbl=0), 0.00),               # [N+](-*)(-*)(-*)-*
    _one(dict(el=_N, arom=0, q=1, h=0), 3.01),                        # [N+](-*)(-*)=*
    _one(dict(el=_N, arom=0, q=1, h=1, n_dbl=0), 4.44),               # [NH+](-*)(-*)-*
    _one(dict(el=_N, arom=0, q=1, h=1), 13.97),                       # [NH+](-*)=*
    _one(dict(el=_N, arom=0, q=1, h=2, n_dbl=0), 16.61),              # [NH2+](-*)-*
    _one(dict(el=_N, arom=0, q=1, h=2), 25.59),                       # [NH2+]=*
    _one(dict(el=_N, arom=0, q=1, h=3), 27.64),                       # [NH3+]-*
    _one(dict(el=_N, arom=1, q=0, h=0, deg=2), 12.89),                # [n](:*):*
    _one(dict(el=_N, arom=1, q=0, h=0, n_dbl=0, nb_arom=3), 4.41),    # [n](:*)(:*):*
    _one(dict(el=_N, arom=1, q=0, h=0, n_dbl=0), 4.93),               # [n](-*)(:*):*
    _one(dict(el=_N, arom=1, q=0, h=0), 8.39),                        # [n](=*)(:*):*
    _one(dict(el=_N, arom=1, q=0, h=1), 15.79),                       # [nH](:*):*
    _one(dict(el=_N, arom=1, q=1, h=0, nb_arom=3), 4.10),             # [n+](:*)(:*):*
    _one(dict(el=_N, arom=1, q=1, h=0), 3.88),                        # [n+](-*)(:*):*
    _one(dict(el=_N, arom=1, q=1, h=1), 14.14),                       # [nH+](:*):*
    _one(dict(el=_N), 26.02),                                         # any other N: as [NH2]-*
    _one(dict(el=_O, arom=1), 13.14),                                 # [o](:*):*
    _one(dict(el=_O, h=0, n_dbl=0, ring3=1), 12.53),                  # [O]1-*-*-1
    _one(dict(el=_O, h=0, n_dbl=0), 9.23),                            # [O](-*)-*
    _one(dict(el=_O, h=0), 17.07),                                    # [O]=*
    _one(dict(el=_O), 20.23),                                         # [OH]-* and any other O
    _one({}, 0.0),                                                    # every other element
]
TPSA = PropertyTable('tpsa', _rows(_TPSA, 0))

# Ertl's S and P contributions, for those who want the variant with them: add TPSA_SP to the tables and the two sums.
_TPSA_SP = [
    _one(dict(el=_S, arom=1, n_dbl=0), 28.24),                        # [s](:*):*
    _one(dict(el=_S, arom=1), 21.70),                                 # [s](=*)(:*):*
    _one(dict(el=_S, arom=0, h=1), 38.80),                            # [SH]-*
    _one(dict(el=_S, arom=0, h=0, n_dbl=0), 25.30),                   # [S](-*)-*
    _one(dict(el=_S, arom=0, h=0, n_dbl=1, deg=1), 32.09),            # [S]=*
    _one(dict(el=_S, arom=0, h=0, n_dbl=1), 19.21),                   # [S](-*)(-*)=*
    _one(dict(el=_S, arom=0, h=0, n_dbl=2), 8.38),                    # [S](-*)(-*)(=*)=*
    _one(dict(el=_S), 25.30),                                         # any other S: as [S](-*)-*
    _one(dict(el=_P, h=0, n_dbl=0), 13.59),                           # [P](-*)(-*)-*
    _one(dict(el=_P, h=0, n_dbl=1, deg=2), 34.14),                    # [P](-*)=*
    _one(dict(el=_P, h=0, n_dbl=1), 9.81),                            # [P](-*)(-*)(-*)=*
    _one(dict(el=_P, h=1, n_dbl=1), 23.47),                           # [PH](-*)(-*)=*
    _one(dict(el=_P), 13.59),                                         # any other P: as [P](-*)(-*)-*
    _one({}, 0.0),
]
TPSA_SP = PropertyTable('tpsa_sp', _rows(_TPSA_SP, 0))

# Wildman-Crippen-style atom contributions: (logP, MR) of the atom and of each of its hydrogens.  The hydrogen types: H1 on carbon,
# H2 on an alcohol O, H3 on N, H4 on an acid / enol O (an OH whose neighbour has a double bond to N, O, P or S), HS elsewhere.
_H1, _H2, _H3, _H4, _HS = (0.1230, 1.057), (-0.2677, 1.395), (0.2142, 0.9627), (0.2980, 1.805), (0.1125, 1.112)


def _wc(f, logp, mr, h):                                              # a row spec with the two value columns (logP, MR)
    return f, ((logp, h[0]), (mr, h[1]))


_SP3 = dict(el=_C, arom=0, n_dbl=0, triple=0)
# Merged, because the word does not tell them apart -- the published types on the left take the one value on the right:
#   C14..C17 (aromatic C bearing F / Cl / Br / I) -> C15;  C19, C20 (aromatic C with three aromatic neighbours, fused or biaryl) -> C19;
#   C22, C23 (aromatic C bearing N / O, also a ring N or O next to a substituted C) -> C22;  C13 and C24 (bearing S, P, B, Si) -> C24;
#   C9 (methyl on an aromatic heteroatom) -> C8;  C27 -> C4;  O9, O10, O11 (carbonyl O by what else its carbon bears) -> O10;
#   O6, O7 and the =O of P -> O6;  O12 and every anion type are left out (no negative charge);  N12, N10: the MR of N11 / NS;
#   Hal (ionic halogen) is left out;  B and Si take Me1.
_WC = [
    # aliphatic carbon
    _wc(dict(el=_C, arom=0, triple=1), 0.0017, 3.888, _H1),                                     # C7
    _wc(dict(el=_C, arom=0, dbl_het=1), -0.2783, 5.007, _H1),                                   # C5
    _wc(dict(**_SP3, nb_het=0, nb_arom=0, h=0), 0.0000, 2.433, _H1),                            # C2
    _wc(dict(**_SP3, nb_het=0, nb_arom=0, h=1), 0.0000, 2.433, _H1),                            # C2
    _wc(dict(**_SP3, nb_het=0, nb_arom=0), 0.1441, 2.503, _H1),                                 # C1
    _wc(dict(**_SP3, nb_het=0, h=3), 0.08452, 2.464, _H1),                                      # C8
    _wc(dict(**_SP3, nb_het=0, h=2), -0.0516, 2.488, _H1),                                      # C10
    _wc(dict(**_SP3, nb_het=0, h=1), 0.1193, 2.582, _H1),                                       # C11
    _wc(dict(**_SP3, nb_het=0), -0.0967, 2.576, _H1),                                           # C12
    _wc(dict(**_SP3, h=3), -0.2035, 2.753, _H1),                                                # C3
    _wc(dict(**_SP3, h=2), -0.2035, 2.753, _H1),                                                # C3
    _wc(dict(**_SP3), -0.2051, 2.731, _H1),                                                     # C4
    _wc(dict(el=_C, arom=0, nb_arom=0), 0.1551, 3.513, _H1),                                    # C6
    _wc(dict(el=_C, arom=0), 0.2640, 4.305, _H1),                                               # C26
    # aromatic carbon
    _wc(dict(el=_C, arom=1, h=0, n_dbl=0, nb_hal=0, nb_arom=3), 0.2955, 4.346, _H1),            # C19
    _wc(dict(el=_C, arom=1, h=0, n_dbl=0, nb_hal=0, nb_het=0), 0.1360, 3.509, _H1),             # C21
    _wc(dict(el=_C, arom=1, h=0, n_dbl=0, nb_hal=0, nb_no=0), 0.1600, 2.673, _H1),              # C24
    _wc(dict(el=_C, arom=1, h=0, n_dbl=0, nb_hal=0), 0.1539, 4.067, _H1),                       # C22
    _wc(dict(el=_C, arom=1, h=0, n_dbl=0), 0.2450, 3.564, _H1),                                 # C15
    _wc(dict(el=_C, arom=1, h=0), 0.0000, 3.135, _H1),                                          # C25
    _wc(dict(el=_C, arom=1), 0.1581, 3.350, _H1),                                               # C18
    # nitrogen
    _wc(dict(el=_N, arom=1, q=0), -0.3239, 2.202, _H3),                                         # N11
    _wc(dict(el=_N, arom=1), -1.119, 2.202, _H3),                                               # N12
    _wc(dict(el=_N, q=1, h=0, n_dbl=0, triple=0), -0.3396, 0.2604, _H3),                        # N13
    _wc(dict(el=_N, q=1, h=0), 0.2887, 3.359, _H3),                                             # N14
    _wc(dict(el=_N, q=1), -1.950, 2.134, _H3),                                                  # N10
    _wc(dict(el=_N, triple=1), -1.566, 1.725, _H3),                                             # N9
    _wc(dict(el=_N, n_dbl=0, h=2, nb_arom=0), -1.019, 2.262, _H3),                              # N1
    _wc(dict(el=_N, n_dbl=0, h=2), -1.027, 2.827, _H3),                                         # N3
    _wc(dict(el=_N, n_dbl=0, h=1, nb_arom=0), -0.7096, 2.173, _H3),                             # N2
    _wc(dict(el=_N, n_dbl=0, h=1), -0.5188, 3.000, _H3),                                        # N4
    _wc(dict(el=_N, n_dbl=0, h=0, nb_arom=0), -0.3187, 1.839, _H3),                             # N7
    _wc(dict(el=_N, n_dbl=0, h=0), -1.239, 2.819, _H3),                                         # N8
    _wc(dict(el=_N, h=0), 0.1836, 2.428, _H3),                                                  # N6
    _wc(dict(el=_N, n_dbl=1), 0.08387, 1.757, _H3),                                             # N5
    # oxygen
    _wc(dict(el=_O, arom=1), 0.1552, 1.080, _H2),                                               # O1
    _wc(dict(el=_O, n_dbl=0, h=0, nb_het=0), -0.0684, 1.085, _H2),                              # O3
    _wc(dict(el=_O, n_dbl=0, h=0), -0.4195, 1.182, _H2),                                        # O4
    _wc(dict(el=_O, n_dbl=0, nb_dbl_het=1), -0.2893, 0.8238, _H4),                              # O2, acid
    _wc(dict(el=_O, n_dbl=0), -0.2893, 0.8238, _H2),                                            # O2
    _wc(dict(el=_O, nb_no=0, nb_het=0, nb_arom=0), 0.1129, 0.2215, _H2),                        # O10
    _wc(dict(el=_O, nb_no=0, nb_het=0), 0.1788, 3.135, _H2),                                    # O8
    _wc(dict(el=_O, nb_no=0), -0.3339, 0.7774, _H2),                                            # O6
    _wc(dict(el=_O, n_dbl=1), 0.0335, 3.367, _H2),                                              # O5
    # sulfur by kind, then one catch-all row per element
    _wc(dict(el=_S, arom=1), 0.6237, 6.691, _HS),                                               # S3
    _wc(dict(el=_S, q=1), -0.0024, 7.365, _HS),                                                 # S2
    _wc(dict(el=_C), 0.08129, 3.243, _H1), _wc(dict(el=_N), -0.4458, 2.134, _H3), _wc(dict(el=_O), -0.1188, 0.6865, _H2),   # CS, NS, OS
    _wc(dict(el=_F), 0.4202, 1.108, _HS), _wc(dict(el=_CL), 0.6895, 5.853, _HS), _wc(dict(el=_BR), 0.8456, 8.927, _HS),
    _wc(dict(el=_I), 0.8857, 14.02, _HS), _wc(dict(el=_P), 0.8612, 6.920, _HS),
    _wc(dict(el=_S), 0.6482, 7.591, _HS),                                                       # S1
    _wc(dict(el=_B), -0.3808, 5.754, _HS), _wc(dict(el=_SI), -0.3808, 5.754, _HS),              # Me1
]
LOGP = PropertyTable('logp', _rows(_WC, 0))
MR = PropertyTable('mr', _rows(_WC, 1))
DEFAULT_TABLES = (TPSA, LOGP, MR)


def _check_tables(who, tables):
    tables = tuple(tables) if isinstance(tables, (list, tuple)) else tables
    if not isinstance(tables, tuple) or not all(isinstance(t, PropertyTable) for t in tables):
        raise ValueError(f'{who}: tables must be a sequence of PropertyTable, not {tables!r}')
    if len(tables) > MAX_TABLES:
        raise ValueError(f'{who}: {len(tables)} tables, at most MAX_TABLES = {MAX_TABLES} go in one call')
    names = [t.name for t in tables]
    if len(set(names)) != len(names):
        raise ValueError(f'{who}: two tables share a name: {names}')
    return tables


def _bounds(who, name, pair, unit):
    """(lo, hi) of a limit as int32 in the kernel's unit, INT_MIN / INT_MAX for none; `pair` is None or (min, max), each a number or None."""
    if pair is None:
        return _INT_MIN, _INT_MAX
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise ValueError(f'{who}: {name} must be None or (min, max), each a number or None, not {pair!r}')
    out = []
    for x, none in zip(pair, (_INT_MIN, _INT_MAX)):
        if x is None:
            out.append(none)
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x):
            raise ValueError(f'{who}: {name} must be None or (min, max), each a finite number or None, not {pair!r}')
        v = round(float(x) * unit)
        if not _INT_MIN < v < _INT_MAX:
            raise ValueError(f'{who}: {name} bound {x!r} does not fit the kernel\'s int32 in units of 1/{unit}')
        out.append(v)
    if out[0] > out[1]:
        raise ValueError(f'{who}: {name} has min above max: {pair!r}')
    return out[0], out[1]


@dataclass(frozen=True)
class PropertyLimits:
    """Limits of the property verdict: None or (min, max) -- each a number or None -- for mol_weight, heavy_atoms, nhoh, no_count and
    rotatable, and in `sums` per table name, e.g. sums={'logp': (None, 5.0)}.  A quantity below its min or above its max is violated
    (the bounds themselves pass); PROP_LIMITS is set when more than `max_violations` quantities are.  A bound is converted to the
    kernel's integer unit once, with `round`: 1e-3 for the weight, 1e-4 for a sum.  The default has no limit at all: only a graph
    without a Kekulé structure fails."""
    mol_weight: tuple = None
    heavy_atoms: tuple = None
    nhoh: tuple = None
    no_count: tuple = None
    rotatable: tuple = None
    sums: dict = field(default_factory=dict)
    max_violations: int = 0

    def __post_init__(self):
        who = 'PropertyLimits'
        for k in LIMITED:
            _bounds(who, k, getattr(self, k), WEIGHT_UNIT if k == 'mol_weight' else 1)
        if not isinstance(self.sums, dict) or not all(isinstance(k, str) for k in self.sums):
            raise ValueError(f'{who}: sums must be a dict {{table name: (min, max)}}, not {self.sums!r}')
        object.__setattr__(self, 'sums', dict(self.sums))
        for k, pair in self.sums.items():
            _bounds(who, f'sums[{k!r}]', pair, SUM_UNIT)
        M._check_int(who, 'max_violations', self.max_violations, 0, 0x7fffffff)

    @classmethod
    def lipinski(cls):
        """Lipinski's rule of five: weight <= 500, logp <= 5, nhoh <= 5, no_count <= 10; one violation is allowed."""
        return cls(mol_weight=(None, 500.0), nhoh=(None, 5), no_count=(None, 10), sums={'logp': (None, 5.0)}, max_violations=1)

    @classmethod
    def veber(cls):
        """Veber's rule: rotatable <= 10 and tpsa <= 140."""
        return cls(rotatable=(None, 10), sums={'tpsa': (None, 140.0)})

    def pairs(self, tables):
        """The int32 (lo, hi) of every limited quantity, [PG_PROP_N_LIMITS][2] in the order of the bits of `violated`, for a call with
        `tables`.  A limit that names a table not among them is a ValueError."""
        names = [t.name for t in tables]
        for k in self.sums:
            if k not in names:
                raise ValueError(f'phoregen_amd.properties: a limit names the table {k!r}, which is not in the call ({names})')
        out = [_bounds('PropertyLimits', k, getattr(self, k), WEIGHT_UNIT if k == 'mol_weight' else 1) for k in LIMITED]
        out += [_bounds('PropertyLimits', k, self.sums.get(k), SUM_UNIT) for k in names]
        return out + [(_INT_MIN, _INT_MAX)] * (hip.PG_PROP_N_LIMITS - len(out))


def violation_names(violated, tables):
    """The names of the set bits of a `violated` word: LIMITED, then the tables' names."""
    names = LIMITED + tuple(t.name for t in tables)
    return tuple(k for i, k in enumerate(names) if int(violated) >> i & 1)


@dataclass
class Properties:
    """Device tensors of one `properties` call; F frames, B graphs, N atom rows."""
    status: torch.Tensor         # int32 [F, B]      PROP_* bits
    counts: torch.Tensor         # int32 [F, B, 16]  PROPERTY_COUNTS
    ok: torch.Tensor             # bool  [F, B]      no bit of PROP_FAIL_MASK
    atom_env: torch.Tensor       # int32 [F, N]      the environment word (`env_fields`); -1: a dropped atom, or no Kekulé structure
    atom_row: torch.Tensor       # uint8 [F, 4, N]   the row taken per table; 255: no row, an unused table, a dropped atom
    sums: torch.Tensor           # int32 [F, B, 4]   the tables' sums in units of 1e-4; unused tables 0
    weight_milli: torch.Tensor   # int32 [F, B]      the weight of the heavy atoms and the hydrogens, times 1000
    violated: torch.Tensor       # int32 [F, B]      bit k: quantity k of LIMITED + the tables' names is outside its limits
    tables: tuple
    limits: PropertyLimits
    screen: M.Screen             # the screen, the Kekulé form and the rings it was computed from
    kekule: M.Kekule
    rings: M.Rings

    @property
    def mol_weight(self):
        """float64 [F, B]"""
        return self.weight_milli.double() / WEIGHT_UNIT

    def value(self, name):
        """The sum of the table `name` as float64 [F, B]."""
        names = [t.name for t in self.tables]
        if name not in names:
            raise ValueError(f'phoregen_amd.properties.Properties.value: no table {name!r} in this call ({names})')
        return self.sums[..., names.index(name)].double() / SUM_UNIT

    @property
    def fsp3(self):
        """sp3 carbons / carbons as float64 [F, B]; 0 where there is no carbon."""
        c, s = self.counts[..., hip.PG_PROP_C_CARBONS].double(), self.counts[..., hip.PG_PROP_C_SP3_CARBONS].double()
        return torch.where(c > 0, s / c.clamp(min=1), torch.zeros_like(c))


def weight_table():
    """`molecule.ATOMIC_WEIGHT` times 1000 as integers: the eleven classes in ATOM_TYPES order, then hydrogen."""
    return [round(M.ATOMIC_WEIGHT[z] * WEIGHT_UNIT) for z in list(ATOM_TYPES) + [1]]


def pack_tables(tables):
    """The rows of the tables, one table after the other, as int32 [rows, 4] (numpy)."""
    rows = [r for t in tables for r in t.rows]
    return np.array(rows, dtype=np.int64).astype(np.int32).reshape(-1, hip.PG_PROP_ROW_INTS)


@torch.no_grad()
def properties(results, frames='final', screen=None, kekule=None, rings=None, tables=DEFAULT_TABLES, limits=PropertyLimits()):
    """Environment words, table sums, counts, weight and the verdict against `limits` for every decoded (frame, graph) of a `sample` /
    `sample_batch` result, on the device, in one launch (pg_mol_props; DESIGN.md 2.9 "Properties").  Whichever of `screen`, `kekule`
    (a `Kekule`) and `rings` (a `Rings`) is not handed in is computed; all must come from one screen.  No host read beyond the
    screen's.  `ok` fails for a graph without a Kekulé structure, or with more violated limits than limits.max_violations.  The
    shipped tables are written from memory, not checked against RDKit."""
    who = 'phoregen_amd.properties.properties'
    node, _, _, F, _ = M._frames(results, frames)
    dev = node.device
    M._need_cuda('properties', 'the property kernel', dev)
    if not isinstance(limits, PropertyLimits):
        raise ValueError(f'{who}: limits must be a PropertyLimits, not {limits!r}')
    tables = _check_tables(who, tables)
    pairs = limits.pairs(tables)
    if kekule is not None and not isinstance(kekule, M.Kekule) or rings is not None and not isinstance(rings, M.Rings):
        raise ValueError(f'{who}: kekule= must be a Kekule and rings= a Rings')
    sc = M._resolve('properties', results, frames, screen, 'phoregen_amd.properties', kekule=kekule, rings=rings)
    kek = kekule if kekule is not None else M.kekulize(results, frames, screen=sc)
    rg = rings if rings is not None else M.rings(results, frames, screen=sc)
    B, N = len(sc.num_atoms), sc.cls.size(1)
    with torch.cuda.device(dev):
        lib = hip.lib()
        out = dict(status=torch.empty(F, B, dtype=torch.int32, device=dev),
                   counts=torch.empty(F, B, len(PROPERTY_COUNTS), dtype=torch.int32, device=dev),
                   atom_env=torch.empty(F, N, dtype=torch.int32, device=dev),
                   atom_row=torch.empty(F, MAX_TABLES, N, dtype=torch.uint8, device=dev),
                   sums=torch.empty(F, B, MAX_TABLES, dtype=torch.int32, device=dev),
                   weight_milli=torch.empty(F, B, dtype=torch.int32, device=dev), violated=torch.empty(F, B, dtype=torch.int32, device=dev))
        packed = torch.from_numpy(pack_tables(tables)).to(dev)
        weights = torch.tensor(weight_table(), dtype=torch.int32, device=dev)
        _launch_props(lib, sc, kek, rg, B, F, max(sc.num_atoms, default=0), packed, [len(t.rows) for t in tables], weights, pairs,
                      limits.max_violations, out)
    return Properties(ok=(out['status'] & PROP_FAIL_MASK) == 0, tables=tables, limits=limits, screen=sc, kekule=kek, rings=rg, **out)


def _launch_props(lib, sc, kek, rg, B, F, max_n, packed, table_rows, weights, pairs, max_violations, out):
    """pg_mol_props on the current stream; sc, kek, rg: anything with the `Screen`, `Kekule` and `Rings` fields the kernel reads;
    packed: int32 [rows, 4] and weights: int32 [12] on the device; table_rows and pairs: host lists.  A graph above MAX_ATOMS, more
    than MAX_TABLES tables or a table above MAX_ROWS rows is the library's error: nothing is launched and `out` is not written."""
    cls, order = sc.cls, sc.order
    M._check_arrays('properties', cls.device, [
        (cls, torch.int8), (order, torch.int8), (kek.kekule_order, torch.int8), (kek.hcount, torch.uint8), (kek.charge, torch.int8),
        (kek.status, torch.int32), (rg.ring_size, torch.uint8), (rg.atom_ring, torch.uint8), (sc.lig_off, torch.int32),
        (sc.bond_off, torch.int32), (packed, torch.int32), (weights, torch.int32), (out['atom_env'], torch.int32),
        (out['atom_row'], torch.uint8), (out['sums'], torch.int32), (out['counts'], torch.int32), (out['weight_milli'], torch.int32),
        (out['violated'], torch.int32), (out['status'], torch.int32)])
    if (sc.lig_off.numel() != B + 1 or sc.bond_off.numel() != B + 1 or cls.numel() != F * cls.size(-1) or order.numel() != F * order.size(-1)
            or kek.hcount.shape != cls.shape or kek.charge.shape != cls.shape or rg.atom_ring.shape != cls.shape
            or kek.kekule_order.shape != order.shape or rg.ring_size.shape != order.shape or kek.status.numel() != F * B
            or packed.numel() != hip.PG_PROP_ROW_INTS * sum(table_rows) or weights.numel() != hip.PG_PROP_N_WEIGHTS
            or len(pairs) != hip.PG_PROP_N_LIMITS or out['atom_env'].shape != cls.shape
            or out['atom_row'].numel() != MAX_TABLES * cls.numel() or out['sums'].numel() != MAX_TABLES * F * B
            or out['counts'].numel() != len(PROPERTY_COUNTS) * F * B
            or any(out[k].numel() != F * B for k in ('weight_milli', 'violated', 'status'))):
        raise ValueError('phoregen_amd.properties.properties: sizes of the offsets, screen / Kekulé / ring arrays, tables, weights, limits '
                         f'and outputs do not fit {F} frames x {B} graphs, {cls.size(-1)} atom rows, {order.size(-1)} pair rows, '
                         f'{sum(table_rows)} table rows')
    rows_c = (ctypes.c_int * max(len(table_rows), 1))(*table_rows)
    lim_c = (ctypes.c_int * (2 * hip.PG_PROP_N_LIMITS))(*[int(x) for pair in pairs for x in pair])
    hip.check(lib.pg_mol_props(cls.data_ptr(), order.data_ptr(), kek.kekule_order.data_ptr(), kek.hcount.data_ptr(), kek.charge.data_ptr(),
                               kek.status.data_ptr(), rg.ring_size.data_ptr(), rg.atom_ring.data_ptr(), sc.lig_off.data_ptr(),
                               sc.bond_off.data_ptr(), B, F, cls.size(-1), 2 * order.size(-1), max_n, packed.data_ptr(), rows_c,
                               len(table_rows), weights.data_ptr(), lim_c, int(max_violations), out['atom_env'].data_ptr(),
                               out['atom_row'].data_ptr(), out['sums'].data_ptr(), out['counts'].data_ptr(),
                               out['weight_milli'].data_ptr(), out['violated'].data_ptr(), out['status'].data_ptr(), hip.stream_ptr()),
              'pg_mol_props')


def status_names(status):
    return tuple(name for bit, name in PROP_NAMES.items() if status & bit)


def molecule_entry(tables, status, counts, sums, weight_milli, violated, env, row):
    """A molecule's 'properties' dict from its rows of the outputs (numpy): counts [16], sums [4], env [n] and row [n, 4] of its
    kept atoms.  'mol_weight', one entry per table name and 'fsp3' are floats; 'violated' is the word, 'violated_names' its names."""
    c = {k: int(x) for k, x in zip(PROPERTY_COUNTS[:-1], counts)}
    out = dict({'status': int(status), 'properties_ok': (int(status) & PROP_FAIL_MASK) == 0}, **c, mol_weight=int(weight_milli) / WEIGHT_UNIT)
    out.update((t.name, int(s) / SUM_UNIT) for t, s in zip(tables, sums))
    out.update(fsp3=c['sp3_carbons'] / c['carbons'] if c['carbons'] else 0.0, violated=int(violated),
               violated_names=violation_names(violated, tables), env=np.asarray(env).astype(np.int32).copy(),
               row=np.asarray(row).astype(np.uint8)[:, :len(tables)].copy())
    return out


def sdf_item(pr):
    """The PHOREGEN_PROPERTIES data item of a molecule's 'properties' dict (`molecule.write_sdf`): the status, the weight with three
    decimals, every table's sum and fsp3 with four, the counts, and the names of the violated quantities ('-' for none)."""
    taken = set(PROPERTY_COUNTS) | {'status', 'properties_ok', 'mol_weight', 'fsp3', 'violated', 'violated_names', 'env', 'row'}
    return ('> <PHOREGEN_PROPERTIES>\nstatus 0x%02x\nmol_weight %.3f\n' % (int(pr['status']), pr['mol_weight'])
            + ''.join('%s %.4f\n' % (k, v) for k, v in pr.items() if k not in taken) + 'fsp3 %.4f\n' % pr['fsp3']
            + ''.join('%s %d\n' % (k, pr[k]) for k in PROPERTY_COUNTS[:-1])
            + 'violated %s\n\n' % (' '.join(pr['violated_names']) or '-'))


def _read(value):
    """`sample_valid(properties=)`: True (the default tables, no limit), a `PropertyLimits` (the default tables), or (tables, limits)."""
    if value is False:
        return None
    opt = (DEFAULT_TABLES, PropertyLimits()) if value is True else (DEFAULT_TABLES, value) if isinstance(value, PropertyLimits) else value
    if not (isinstance(opt, tuple) and len(opt) == 2 and isinstance(opt[1], PropertyLimits)):
        raise ValueError('phoregen_amd.molecule.sample_valid: properties= must be True, a PropertyLimits or (tables, PropertyLimits), '
                         f'not {value!r}')
    tables = _check_tables('phoregen_amd.molecule.sample_valid', opt[0])
    opt[1].pairs(tables)                                               # (a limit on a table that is not in the call: now, not in the first draw)
    return tables, opt[1]


def _atoms_of_rows(at, a):
    """The kept atoms' columns of a per-table, per-atom view [4, N], as [n, 4]."""
    return a[:, at.n0:at.n0 + at.n][:, at.keep].T


# What `molecule.assemble`, `write_sdf` and `sample_valid` know about this analysis.
ANALYSIS = M._Analysis(
    'properties', 'properties', Properties,
    parts=lambda x: [('d_status', x.status[0], np.int32), ('d_counts', x.counts[0], np.int32), ('d_sums', x.sums[0], np.int32),
                     ('d_weight', x.weight_milli[0], np.int32), ('d_violated', x.violated[0], np.int32), ('d_env', x.atom_env[0], np.int32),
                     ('d_row', x.atom_row[0], np.uint8)],
    entry=lambda x, v, at, mol: {'properties': molecule_entry(x.tables, at.row(v['d_status']), at.row(v['d_counts']), at.row(v['d_sums']),
                                                              at.row(v['d_weight']), at.row(v['d_violated']), at.atoms(v['d_env']),
                                                              _atoms_of_rows(at, v['d_row']))},
    sdf=lambda m: sdf_item(m['properties']), read=_read,
    compute=lambda d, opt: properties(d.res, screen=d.screen, kekule=d.of('kekule'), rings=d.of('rings'), tables=opt[0], limits=opt[1]),
    verdict=lambda m: m['properties']['properties_ok'])
