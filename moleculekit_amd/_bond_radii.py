"""Radii by element, in Angstrom, for the bond guesser (bonds.py): the values the reference's ``moleculekit.bondguesser`` looks
elements up in -- Bondi's van der Waals radii (J. Phys. Chem. 68, 441, 1964) with hydrogen at 1.0 A (J. Phys. Chem. 100, 7384, 1996),
CHARMM27 ion radii for Na, Mg, K, Ca and Zn among others, and 2.0 A where nothing is tabulated.

The keys are capitalised element symbols.  An upper-case symbol such as "CL" is NOT in the table: the guesser then falls through to
the default of the atom name's first letter (``NAME_DEFAULTS``) and from there to ``FALLBACK``, as the reference does.

H, C, N, O and S are checked against the bonds of tests/golden/channels_3ptb.npz (tests/test_bonds_cpu.py); Cl through the seeded
pair cases.
"""

_TWO = ("Be B Al Sc Ti V Cr Mn Fe Co Ge Rb Sr Y Zr Nb Mo Tc Ru Rh Sb Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Bi "
        "Po At Rn Fr Ra Ac Th Pa Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg").split()

BOND_RADII = {
    "H": 1.0, "He": 1.4, "Li": 1.82, "C": 1.7, "N": 1.55, "O": 1.52, "F": 1.47, "Ne": 1.54, "Na": 1.36, "Mg": 1.18, "Si": 2.1, "P": 1.8,
    "S": 1.8, "Cl": 2.27, "Ar": 1.88, "K": 1.76, "Ca": 1.37, "Ni": 1.63, "Cu": 1.4, "Zn": 1.39, "Ga": 1.07, "As": 1.85, "Se": 1.9, "Br": 1.85,
    "Kr": 2.02, "Pd": 1.63, "Ag": 1.72, "Cd": 1.58, "In": 1.93, "Sn": 2.17, "Te": 2.06, "I": 1.98, "Xe": 2.16, "Cs": 2.1, "Pt": 1.72,
    "Au": 1.66, "Hg": 1.55, "Tl": 1.96, "Pb": 2.02, "U": 1.86,
}
BOND_RADII.update({el: 2.0 for el in _TWO})

NAME_DEFAULTS = {"H": 1.0, "C": 1.5, "N": 1.4, "O": 1.3, "F": 1.2, "S": 1.9}     # by the upper-cased first letter of the atom NAME
FALLBACK = 1.5
