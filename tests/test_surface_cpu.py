"""CPU: the Python recognise surface does with its arguments what tests/golden/surface.json recorded before ``Engine``'s four
recognise methods and ``MangaOcr``'s sources x results grid were each folded into one request path - the C symbol chosen,
position, nullness and value of every argument, the engine keywords of every ``MangaOcr`` method (only the ones somebody
asked for), what comes back, and the type, message and order of every refusal.  tests/golden/make_surface_golden.py is both
the recorder and the description of what is recorded; this test runs its ``record()`` again and compares the digests, one
per method (``python tests/golden/make_surface_golden.py --show GROUP`` prints a group's scenarios in full)."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def surface():
    spec = importlib.util.spec_from_file_location("make_surface_golden", os.path.join(GOLDEN, "make_surface_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.PATH, "r", encoding="ascii") as f:
        want = json.load(f)
    rec = mod.record()
    return want, mod.digest(rec), rec


@pytest.mark.parametrize("section", ["engine", "ocr", "errors"])
def test_the_surface_is_the_recorded_one(surface, section):
    want, got, _ = surface
    assert list(got[section]) == list(want[section]), "the scenarios themselves changed: regenerate only with a reason"
    changed = [g for g in want[section] if got[section][g] != want[section][g]]
    assert not changed, f"{len(changed)} of {len(want[section])} methods do not behave as recorded: {changed[:8]} (--show GROUP prints the scenarios)"


def test_the_recording_covers_every_public_recognise_method(surface):
    want, _, rec = surface
    from manga_ocr.ocr import MangaOcr
    words = {w for name in list(rec["ocr"]) + list(rec["errors"]) for w in name.replace("[", " ").split()}
    public = [m for m in dir(MangaOcr) if m.startswith(("recognize", "score_")) and m not in ("recognize_page", "recognize_pages")]
    assert len(public) >= 27 and not [m for m in public if m not in words], "a public method without a recorded scenario"
    for kind in ("images", "regions", "gray_host", "device"):
        for variant in ("positions", "prefix", "shared", "beam"):
            assert any(c["symbol"] == f"mocr_recognize_{kind}_{variant}" for e in rec["engine"].values() for c in e["calls"])
    assert sum(n for groups in want.values() for n, _ in groups.values()) == sum(len(e) for e in rec.values()) > 1300
