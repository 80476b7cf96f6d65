"""CPU test of the baked march entries' refusals, word for word: every call of tools/make_baked_refusals.py (each single defect that
test_baked_host.py, test_baked_sh_host.py, test_sparse_baked_host.py and test_baked_half_host.py exercise, on every entry, and a few
pairs that pin the order of the checks) gives the return code and the full pnr_last_error() that the fixture recorded at the commit
before the entries shared one checked description.  No call reaches a launch: it is refused, or it has no rays."""
import importlib.util
import json
import os

from pixelnerf_amd import _lib


def _tool(repo_root):
    spec = importlib.util.spec_from_file_location("make_baked_refusals", os.path.join(repo_root, "tools", "make_baked_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_refusal_of_every_baked_entry_keeps_its_words(repo_root):
    tool = _tool(repo_root)
    want = json.load(open(tool.FIXTURE))
    assert sorted(want) == sorted(tool.ENTRIES) and len(want) == 10
    assert all(name in _lib.PROTOTYPES for name in want)
    # the fixture itself: nothing in it was launched, and every message names its entry
    for name, calls in want.items():
        assert len(calls) >= 40
        for label, (rc, message) in calls.items():
            assert (rc, message) == (0, "") and "no rays" in label or rc == -1 and message.startswith(name + ": "), (name, label)
    got = tool.record(_lib.load())
    for name in want:
        assert sorted(got[name]) == sorted(want[name]), name
        for label in want[name]:
            assert got[name][label] == want[name][label], (name, label, got[name][label], want[name][label])
