"""Standard atomic weights by element, in unified atomic mass units, for the mass-weighted group moments (moments.py): the IUPAC
table "Atomic weights of the elements 2001" (Pure Appl. Chem. 75, 1107-1122, 2003) -- the generation of values the reference's
periodic table holds, which is what its MetricCoordinate(groupreduce="com") and MetricGyration (where a molecule carries no
masses) look elements up in.

H, C, N, O, S and Cl are checked: their float32 values equal the per-element masses the golden generator recorded from the reference
for the elements of the fixture (tests/test_moments_cpu.py); every other entry is listed in DESIGN.md section 12 as unchecked.  An
element that is not here raises KeyError.
"""

ATOMIC_MASSES = {
    "H": 1.00794, "He": 4.002602, "Li": 6.941, "Be": 9.012182, "B": 10.811, "C": 12.0107, "N": 14.0067, "O": 15.9994,
    "F": 18.9984032, "Ne": 20.1797, "Na": 22.989770, "Mg": 24.3050, "Al": 26.981538, "Si": 28.0855, "P": 30.973761, "S": 32.065,
    "Cl": 35.453, "Ar": 39.948, "K": 39.0983, "Ca": 40.078, "Mn": 54.938049, "Fe": 55.845, "Co": 58.933200, "Ni": 58.6934,
    "Cu": 63.546, "Zn": 65.409, "Se": 78.96, "Br": 79.904, "I": 126.90447,
}

CHECKED = ("H", "C", "N", "O", "S", "Cl")


def masses_for(elements):
    """list of masses (u) for an iterable of element symbols; KeyError for an element without an entry"""
    return [ATOMIC_MASSES[str(e)] for e in elements]
