"""CPU tier: WHICH path a lattice call takes.

All of run_lattice's paths (csrc/pipeline.h: the one-launch pre-passes, the kernel chain, direct binning in front of it; the
plain, lean, team and workgroup-per-item tile kernels; the split exact fix-up) compute the same bits by design, so the value
tests of test_emu_kernels.py cannot see a call that quietly moves from one to another -- only a GPU timing can.  Here
run_lattice drives a backend that records instead of running (tests/emu/emu_capi.cpp, RecBackend): every workspace request
(slot, set, bytes), every memset, every launch (kernel instantiation, grid, block, each argument as the buffer it points
into) and the counter book-keeping the call leaves behind.  The traces are compared with tests/golden/lattice_paths.txt.

The fixture is a record of what the host code does, not a statement of what it should do: a change that means to move a call
to another path, or to resize a buffer, regenerates it (python -m tests.test_lattice_paths --write) and the diff of the
fixture shows exactly which calls changed and how.  A refactor of the host code leaves it untouched.
"""
import os
import sys

import pytest

from tests import emu_build as emu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lattice_paths.txt")

# 24^3 voxels of 1 A: 125 cells, 54 tiles of K = 4 per item; <= 18 such items are a "team" launch (<= 1 024 tile waves)
ONE = dict(B=1, total_atoms=3000)                       # one molecule per call: the one-launch pre-pass k_bin_solo + the team kernel
MID = dict(B=64, total_atoms=64 * 300)                  # a batch of small items: the per-item pre-pass
CHAIN = dict(B=24, total_atoms=24 * 5000)               # items of more than 4 096 atoms: the kernel chain
BIG = dict(B=40, total_atoms=40 * 6000)                 # >= 200 000 atoms: pipelined where possible, else direct binning in front of the chain
LIG = dict(B=4096, total_atoms=4096 * 60)               # ligand-sized items: a workgroup per item
TOPO = dict(B=64, total_atoms=64 * 3000, topo=1)        # frames of one molecule

CASES = {
    # ---- nothing to do, refusals ----
    "no_items": dict(B=0),
    "no_voxels": dict(ONE, nx=0),
    "no_channels": dict(ONE, C=0),
    "no_atoms": dict(B=2, total_atoms=0),
    "no_atoms_chain": dict(B=2, total_atoms=0, prepass_mode=0),
    "no_atoms_general_chain": dict(B=2, total_atoms=0, prepass_mode=0, force_general=1),
    # ---- one molecule: k_bin_solo, the team kernel ----
    "one_f32": dict(ONE),
    "one_f64": dict(ONE, sigmas_f64=1),
    "one_twice": dict(ONE, calls=2),
    "one_seq": dict(ONE, seq=7),
    "one_direct0": dict(ONE, direct=0),
    "one_prepass0": dict(ONE, prepass_mode=0),
    "one_prepass1": dict(ONE, prepass_mode=1),
    "one_team0": dict(ONE, tile_team=0),
    "one_team1": dict(ONE, tile_team=1),
    "one_team4": dict(ONE, tile_team=4),
    "one_team8": dict(ONE, tile_team=8),
    "one_team16": dict(ONE, tile_team=16),
    "one_team16_k8": dict(ONE, tile_team=16, tile_k=8),
    "one_k8": dict(ONE, tile_k=8),
    "one_items1": dict(ONE, tile_items=1),
    "one_general": dict(ONE, force_general=1),
    "one_fine_cells": dict(ONE, fine_cells=1),
    "one_two_groups": dict(ONE, C=12),
    "one_periodic": dict(ONE, pbc=1, max_images=2),
    "one_tier1": dict(ONE, lds_tier=1),
    "one_tier2": dict(ONE, lds_tier=2),
    "one_tier9": dict(ONE, lds_tier=9),
    "one_cell_cap_2048": dict(ONE, cell_cap=2048),
    "one_half_angstrom": dict(ONE, nx=48, ny=48, nz=48, voxelsize=0.5),
    "one_million_atoms": dict(B=1, total_atoms=1100000),
    "one_million_atoms_chain": dict(B=1, total_atoms=1100000, direct=0),
    "one_topo": dict(ONE, topo=1, topo_wide=2),
    # ---- a few ligand-sized items: team launch, per-item pre-pass ----
    "few_ligands": dict(B=8, total_atoms=8 * 60),
    "few_ligands_team1": dict(B=8, total_atoms=8 * 60, tile_team=1),
    "few_ligands_items0": dict(B=8, total_atoms=8 * 60, tile_items=0),
    "ligands_32": dict(B=32, total_atoms=32 * 60),
    # ---- batches of small items: k_prepass_items ----
    "mid": dict(MID),
    "mid_f64": dict(MID, sigmas_f64=1),
    "mid_twice": dict(MID, calls=2),
    "mid_periodic": dict(MID, pbc=1, max_images=2),
    "mid_general": dict(MID, force_general=1),
    "mid_items1": dict(MID, tile_items=1),
    "mid_items1_tier1": dict(MID, tile_items=1, lds_tier=1),
    "mid_team1": dict(MID, tile_team=1),
    "mid_direct2": dict(B=32, total_atoms=32 * 500, direct=2),
    "mid_direct2_f64": dict(B=32, total_atoms=32 * 500, direct=2, sigmas_f64=1),
    "mid_prepass0_65": dict(B=65, total_atoms=65 * 300, prepass_mode=0),      # 65 x 126 = 8 190 cells: k_prepass_small
    "mid_prepass0_66": dict(B=66, total_atoms=66 * 300, prepass_mode=0),      # 8 316 > SMALL_PREPASS_MAX_CELLS: the reduce chain
    "mid_hist_2048": dict(MID, nx=64, ny=64, nz=64),
    "mid_hist_2048_f64": dict(MID, nx=64, ny=64, nz=64, sigmas_f64=1),
    "mid_hist_8192": dict(B=8, total_atoms=8 * 300, nx=128, ny=128, nz=128),
    "mid_hist_8192_f64": dict(B=8, total_atoms=8 * 300, nx=128, ny=128, nz=128, sigmas_f64=1),
    "mid_hist_too_big": dict(B=8, total_atoms=8 * 300, nx=160, ny=160, nz=160),
    "big_items_prepass1": dict(B=4, total_atoms=4 * 10000, prepass_mode=1),
    "ligands": dict(LIG),
    "ligands_items0": dict(LIG, tile_items=0),
    "ligands_tier2_feedback": dict(LIG, feedback=(900, 800, 0, 1000)),
    "ligands_100": dict(B=2048, total_atoms=2048 * 100),
    "ligands_pipelining": dict(LIG, pipelining=1),
    # ---- the kernel chain ----
    "chain": dict(CHAIN),
    "chain_f64": dict(CHAIN, sigmas_f64=1),
    "chain_twice": dict(CHAIN, calls=2),
    "chain_periodic": dict(CHAIN, pbc=1, max_images=2),
    "chain_periodic_f64": dict(CHAIN, pbc=1, max_images=2, sigmas_f64=1),
    "chain_general": dict(CHAIN, force_general=1),
    "chain_value_tol": dict(CHAIN, value_tol=1e-6),
    "chain_two_groups": dict(CHAIN, C=12),
    "chain_seq": dict(CHAIN, seq=3),
    "chain_tier1_feedback": dict(CHAIN, feedback=(100, 0, 0, 1000)),
    "chain_tier2_feedback": dict(CHAIN, feedback=(100, 100, 0, 1000)),
    "chain_tier0_feedback": dict(CHAIN, feedback=(50, 0, 0, 1000)),
    "chain_direct1": dict(CHAIN, direct=1),
    "chain_direct1_f64": dict(CHAIN, direct=1, sigmas_f64=1),
    "chain_direct1_twice": dict(CHAIN, direct=1, calls=2),
    "chain_direct1_caps": dict(CHAIN, direct=1, cell_cap=16, spill_cap=64),
    "chain_direct1_periodic": dict(CHAIN, direct=1, pbc=1, max_images=2),
    "chain_direct1_capped_grids": dict(B=256, total_atoms=256 * 5000, direct=1),
    "chain_k4_forced": dict(BIG, nx=48, ny=48, nz=48, tile_k=4),
    # ---- either side of 200 000 atoms, with and without pipelining ----
    "big_in_order": dict(BIG),
    "big_in_order_f64": dict(BIG, sigmas_f64=1),
    "big_direct0": dict(BIG, direct=0),
    "big_pipelined": dict(BIG, pipelining=1, calls=3),
    "big_pipelined_direct1": dict(BIG, pipelining=1, direct=1),
    "big_pipelined_tier1": dict(BIG, pipelining=1, lds_tier=1),
    "big_pipelined_tier2": dict(BIG, pipelining=1, lds_tier=2),
    "big_pipelined_k8_no_hurry": dict(BIG, pipelining=1, nx=48, ny=48, nz=48),
    "big_pipelined_periodic": dict(BIG, pipelining=1, pbc=1, max_images=2),
    "below_200k_pipelining": dict(B=40, total_atoms=40 * 4900, pipelining=1),
    "below_200k": dict(B=40, total_atoms=40 * 4900),
    "cfg1_items_pipelining": dict(B=128, total_atoms=128 * 1639, pipelining=1),     # the chain pays: its pre-pass hides
    "cfg1_items": dict(B=128, total_atoms=128 * 1639),
    "cfg1_items_below_200k_pipelining": dict(B=120, total_atoms=120 * 1639, pipelining=1),
    # ---- a topology call ----
    "topo": dict(TOPO),
    "topo_twice": dict(TOPO, calls=2),
    "topo_periodic": dict(TOPO, pbc=1, max_images=2),
    "topo_wide": dict(TOPO, topo_wide=3),
    "topo_wide_f64": dict(TOPO, topo_wide=3, sigmas_f64=1),
    "topo_wide_in_place": dict(TOPO, topo_wide=3, exact_redo_list=-1),
    "topo_wide_in_place_f64": dict(TOPO, topo_wide=3, exact_redo_list=-1, sigmas_f64=1),
    "topo_wide_small_list": dict(TOPO, topo_wide=3, exact_redo_list=5),
    "topo_wide_seq": dict(TOPO, topo_wide=3, seq=9),
    "topo_wide_pipelined": dict(B=80, total_atoms=80 * 3000, topo=1, topo_wide=3, pipelining=1, calls=2),
    "topo_direct1": dict(TOPO, direct=1),
    "topo_prepass1": dict(TOPO, prepass_mode=1),
    "topo_overflow": dict(TOPO, topo_overflow=1),
    "topo_general": dict(TOPO, force_general=1),
    "topo_value_tol": dict(TOPO, value_tol=1e-6),
    "topo_wrong_length": dict(B=64, total_atoms=64 * 3000 + 1, topo=1),
}


def _read_fixture():
    traces, name = {}, None
    with open(FIXTURE) as f:
        for ln in f:
            if ln.startswith("== "):
                name = ln[3:].strip()
                traces[name] = ""
            elif name is not None:
                traces[name] += ln
    return traces


def _trace(case):
    st, text = emu.trace_lattice(**CASES[case])
    return text


def test_the_table_reaches_every_branch():
    """Every pre-pass form, tile-kernel flavour, tier and float / double instance run_lattice can launch occurs in the fixture."""
    text = open(FIXTURE).read()
    for needle in ("k_bin_solo<float>", "k_bin_solo<double>", "k_bin_direct<float>", "k_bin_direct<double>", "k_prepass_small", "k_prepass_reduce1",
                   "k_prepass_items<float, 512>", "k_prepass_items<float, 2048>", "k_prepass_items<float, 8192>", "k_prepass_items<double, 512>",
                   "k_prepass_items<double, 2048>", "k_prepass_items<double, 8192>",
                   "k_bin_count<float, 0, false, false>", "k_bin_count<float, 1, false, false>", "k_bin_count<double, 0, false, false>",
                   "k_bin_count<double, 1, false, false>", "k_bin_count<float, 0, true, false>", "k_bin_count<double, 0, true, false>",
                   "k_bin_count<float, 0, false, true>", "k_bin_count<float, 1, false, true>",
                   "k_bin_fill<float, false, false>", "k_bin_fill<double, false, false>", "k_bin_fill<float, true, false>",
                   "k_bin_fill<double, true, false>", "k_bin_fill<float, false, true>",
                   "k_voxelize_tiles<4, 640>", "k_voxelize_tiles<4, 768>", "k_voxelize_tiles<4, 1024>", "k_voxelize_tiles<8, 640>",
                   "k_voxelize_tiles_lean<4, 640>", "k_voxelize_tiles_lean<4, 768>", "k_voxelize_tiles_lean<8, 640>",
                   "k_voxelize_tiles_team<4, 640, 4>", "k_voxelize_tiles_team<4, 640, 8>", "k_voxelize_tiles_team<4, 640, 16>",
                   "k_voxelize_tiles_team<8, 640, 4>", "k_voxelize_tiles_team<4, 768, 8>", "k_voxelize_tiles_team<4, 1024, 8>", "k_voxelize_items<4>", "k_voxelize_items<8>",
                   "k_tail<4, 640, float>", "k_tail<4, 640, double>", "k_tail<8, 640, float>", "k_exact_shells<float, false>",
                   "k_exact_shells<double, true>", "k_exact_redo<float>", "k_exact_redo<double>", "k_zero_words",
                   "acquire_set 1 -> set 1", "hurry 0", "tail reports"):
        assert needle in text, needle


@pytest.mark.parametrize("case", sorted(CASES))
def test_lattice_call_takes_the_recorded_path(case):
    expected = _read_fixture()
    assert set(expected) == set(CASES), "tests/golden/lattice_paths.txt and CASES name different calls"
    got = _trace(case)
    assert "unknown" not in got, "a launch whose kernel or pointer the recorder cannot name"
    assert got == expected[case]


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        with open(FIXTURE, "w") as f:
            for case in sorted(CASES):
                f.write("== %s\n%s" % (case, _trace(case)))
        print("wrote", FIXTURE)
