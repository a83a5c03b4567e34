"""Both XTC decoders on DAMAGED files, CPU tier: tests/emu/xtc_damage_main.cpp -- the host decoder (csrc/xtc_reader.h), the header parser
(csrc/xtc_headers.h) and the device decoder's kernels (csrc/xtc_gpu.h on the SIMT emulation) compiled into a program of its own with
AddressSanitizer and UndefinedBehaviorSanitizer, run as child processes on the committed fixtures, which it damages itself: header
fields, cut files, every bit of the small streams, the flag and run bits of the large ones, runs of garbage.  Every buffer is a heap
block of exactly the contracted size, so the bounds arguments of xtc_gpu.h (the XS_SPEC records of slack, the dead lanes' refills, XTC_PAD)
are checked by the sanitizer; the verdicts by the driver's own assertions (its head comment lists them).

The driver runs ONCE for this module (29 CPU-minutes dealt to at most 16 processes: about 5 minutes on 8 cores; DESIGN.md has the
counts and what is cut); the tests read its counts."""
import json
import os

import pytest

from tests import emu_xtc_damage_build as drv

# every refusal site of the two decoders and of the parser that the contents of a file can reach.  Not among them, because no file
# reaches them: the walk's limits on atoms (>= 2^21) and stream bytes (>= 512 MB) -- "dev: size limits" is reached through a number
# of more than 64 bits --, decode_frame's final "atoms missing" (it counts atoms read and written together) and the parser's
# "frame outside the bytes handed over" (a caller's error).
SITES = [
    "dev: header smallidx", "dev: e_end", "dev: e_wide", "dev: e_more, atom count", "dev: e_more, next > tot",
    "dev: e_idx, below the table", "dev: e_idx, above the table", "dev: size limits",
    "dev: refusal while the wave looked at groups together", "dev: refusal in a wave with live lanes",
    "host: index: magic of the first frame", "host: index: atom count < 0", "host: index: nbytes < 0",
    "host: frame: magic", "host: frame: first atom count", "host: frame: second atom count", "host: frame: nbytes", "host: frame: range 0",
    "host: frame: header smallidx", "host: stream: more atoms than announced", "host: stream: smallidx below the table",
    "host: stream: smallidx above the table", "host: stream: overrun",
    "host: read: corrupt XTC frame", "host: read: atom count of the file differs from the buffers'", "host: read: cannot open",
    "host: info: cannot open",
    "parser: magic or atom counts", "parser: nbytes", "parser: range 0", "parser: frame index out of range",
]
KINDS = ["header: magic", "header: atom count", "header: precision", "header: range", "header: smallidx", "header: nbytes", "truncation",
         "stream: every bit", "stream: flag bit", "stream: run bit", "stream: bit at a refill", "stream: seeded bit", "stream: garbage run"]
# which damage a site must be reached BY (besides being reached at all): the verdicts that follow from the damage
BY = [("dev: header smallidx", "header: smallidx"), ("host: frame: header smallidx", "header: smallidx"), ("dev: e_wide", "header: smallidx"),
      ("parser: range 0", "header: range"), ("host: frame: range 0", "header: range"), ("dev: size limits", "header: range"),
      ("parser: nbytes", "header: nbytes"), ("host: frame: nbytes", "header: nbytes"), ("host: index: nbytes < 0", "header: nbytes"),
      ("dev: e_end", "header: nbytes"), ("dev: e_more, next > tot", "header: nbytes"),
      ("parser: magic or atom counts", "header: atom count"), ("parser: magic or atom counts", "header: magic"),
      ("parser: frame index out of range", "truncation"), ("dev: e_more, atom count", "stream: run bit"),
      ("dev: e_idx, below the table", "stream: run bit"), ("host: stream: overrun", "stream: flag bit")]

_RESULT = {}


@pytest.fixture(scope="module")
def counts():
    if not _RESULT:
        total, seconds = drv.run()
        _RESULT.update(total=total, seconds=seconds)
        print(f"\n[xtc damage] {total['cases']} cases, {total['runs']} runs of both decoders in {seconds:.0f} s: " +
              ", ".join(f"{k} {v}" for k, v in sorted(total["kinds"].items())))
    return _RESULT["total"]


def test_sanitized_driver_is_clean_and_reaches_every_refusal_site(counts):
    """The driver exits 0 in every process -- no sanitizer report, none of its assertions -- and its table reaches every refusal
    site at least once, each damage kind runs, and the verdicts that follow from a damage come from that damage."""
    for kind in KINDS:
        assert counts["kinds"].get(kind, 0) > 0, kind
    missing = [s for s in SITES if counts["reach"].get(s, 0) <= 0]
    assert not missing, missing
    missing = [f"{s} | {k}" for s, k in BY if counts["reach"].get(f"{s} | {k}", 0) <= 0]
    assert not missing, missing
    unknown = [s for s in counts["reach"] if " | " not in s and s not in SITES]
    assert not unknown, unknown                      # (a site the list above does not know: "dev: ?" would be a refusal without a cause)


def test_listed_cases_are_the_committed_ones(counts):
    """tests/golden/xtc_damage_cases.json (what the GPU tier replays: tests/test_xtc_reference_streams.py) is what the driver lists
    today: the first two cases of every device refusal site, of every damage kind refused by the device, by the parser or dropped
    from the frame index, of the refusals while groups were taken together and in a mixed wave, and of those both decoders accept."""
    with open(drv.CASES_JSON) as f:
        committed = json.load(f)
    assert counts["listed"] == committed
    keys = {}
    for e in committed:
        for k in e["keys"]:
            keys[k] = keys.get(k, 0) + 1
    for site in SITES[:8]:
        assert keys.get(site, 0) == 2, site
    assert keys.get("refusal while together", 0) == 2 and keys.get("refusal in a mixed wave", 0) == 2
    assert sum(v for k, v in keys.items() if k.startswith("accepted by both")) >= 5
    assert 24 <= len(committed) <= 100


def test_fixtures_are_inside_the_repository():
    for fn in drv.FIXTURES:
        assert os.path.exists(fn) and "golden" in fn
