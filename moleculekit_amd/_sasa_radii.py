"""Van der Waals radii by element, in nanometres, for the Shrake-Rupley surface (sasa.py): the values mdtraj's
``mdtraj.geometry.sasa._ATOMIC_RADII`` holds (Bondi / Mantina radii as tabulated at https://en.wikipedia.org/wiki/Atomic_radii_of_the_elements_(data_page);
ionic radii where no van der Waals radius is tabulated there), which is what the reference's MetricSasa looks elements up in.

H, C, N, O and S are checked against the reference's held SASA arrays (tests/test_sasa_cpu.py: one sphere point of a carbon is
0.126 square Angstrom, the tolerance 0.1); every other entry is listed in DESIGN.md section 9 as unchecked.  An element that is
not here raises KeyError, as the reference does.
"""

ATOMIC_RADII = {
    "H": 0.120, "He": 0.140, "Li": 0.076, "Be": 0.059, "B": 0.192, "C": 0.170, "N": 0.155, "O": 0.152, "F": 0.147, "Ne": 0.154,
    "Na": 0.102, "Mg": 0.086, "Al": 0.184, "Si": 0.210, "P": 0.180, "S": 0.180, "Cl": 0.181, "Ar": 0.188, "K": 0.138, "Ca": 0.114,
    "Sc": 0.211, "Ti": 0.200, "V": 0.200, "Cr": 0.200, "Mn": 0.200, "Fe": 0.200, "Co": 0.200, "Ni": 0.163, "Cu": 0.140, "Zn": 0.139,
    "Ga": 0.187, "Ge": 0.211, "As": 0.185, "Se": 0.190, "Br": 0.185, "Kr": 0.202, "Rb": 0.303, "Sr": 0.249, "Pd": 0.163,
    "Ag": 0.172, "Cd": 0.158, "In": 0.193, "Sn": 0.217, "Sb": 0.206, "Te": 0.206, "I": 0.198, "Xe": 0.216, "Cs": 0.167,
    "Ba": 0.149, "Pt": 0.175, "Au": 0.166, "Hg": 0.155, "Tl": 0.196, "Pb": 0.202, "U": 0.186,
}

CHECKED = ("H", "C", "N", "O", "S")


def radii_for(elements):
    """float64 list of radii (nm) for an iterable of element symbols; KeyError for an element without an entry"""
    return [ATOMIC_RADII[str(e)] for e in elements]
