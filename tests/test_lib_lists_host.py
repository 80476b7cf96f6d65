"""The build lists of pixelnerf_amd._lib name every file of csrc: a source that is not in SOURCES is not compiled, and a header that
is not in HEADERS does not count for the rebuild check (a stale library would pass for a fresh one).  No GPU."""
import glob
import os

from pixelnerf_amd import _lib


def _names(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(_lib.CSRC, pattern)))


def test_every_hip_source_is_in_sources():
    assert _names("pnr_*.hip"), "no sources found"
    assert sorted(_lib.SOURCES) == _names("pnr_*.hip")
    assert _names("*.hip") == _names("pnr_*.hip"), "tools/build_objs.sh compiles pnr_*.hip only"


def test_every_header_is_in_headers():
    listed = sorted(h for h in _lib.HEADERS if os.sep not in h)
    assert listed == sorted(_names("*.h") + _names("*.inc"))
    public = [h for h in _lib.HEADERS if os.sep in h]
    assert len(public) == 1 and os.path.exists(os.path.join(_lib.CSRC, public[0])), "the public header"
    assert len(set(_lib.HEADERS)) == len(_lib.HEADERS) and len(set(_lib.SOURCES)) == len(_lib.SOURCES)
