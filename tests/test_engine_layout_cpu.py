"""The engine's layouts against tests/golden/engine_layout.json (written by tests/golden/make_engine_layout.py from the library
of the commit before the layout code was split by concern): packed-weight size, stage ranges, both workspace sizes, and a hash
of the parameter table and of every named workspace offset, for every architecture / dtype / frame count / deterministic flag /
batch.  Host arithmetic only: no GPU."""
import importlib.util
import itertools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_engine_layout", os.path.join(GOLDEN, "make_engine_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_layouts_match_the_recorded_ones():
    mk = _maker()
    with open(os.path.join(GOLDEN, "engine_layout.json")) as f:
        want = json.load(f)
    combos = list(itertools.product(mk.ARCHS, mk.DTYPES, mk.FRAMES, mk.DETERMINISTIC, mk.BATCHES))
    assert sorted(want) == sorted(mk.key(*c) for c in combos)
    bad = []
    for c in combos:
        got, lines = mk.record(*c)
        if got != want[mk.key(*c)]:
            bad.append(mk.key(*c))
            print(f"{mk.key(*c)}\n  recorded {want[mk.key(*c)]}\n  computed {got}")
            if got[4] != want[mk.key(*c)][4]:  # the computed table behind the differing hash
                print("\n".join("    " + ln for ln in lines))
    assert not bad, f"{len(bad)} of {len(combos)} layouts differ from the record: {bad[:8]}"
