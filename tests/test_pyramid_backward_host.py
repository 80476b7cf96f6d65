"""CPU tests of pnr_pyramid_to_latent_backward: declared, exported, bound, ABI revision unchanged, and its host-side
validation is the forward's (no compute calls: every case returns before a launch)."""
import ctypes
import os
import re

import pytest

from pixelnerf_amd import _lib

NAME = "pnr_pyramid_to_latent_backward"
FAKE = 64  # a non-null, 16-byte aligned "device pointer": never dereferenced, every case below returns before a launch


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def backward(lib, shapes, NV, d_latent=FAKE, stage_ptrs=None, nchw=0):
    n = len(shapes)
    ptrs = _ptrs(stage_ptrs if stage_ptrs is not None else [FAKE] * n)
    rc = lib.pnr_pyramid_to_latent_backward(d_latent, nchw, ptrs, _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes]),
                                            _ints([s[2] for s in shapes]), n, NV, None)
    return rc, lib.pnr_last_error()


def forward(lib, shapes, NV):
    n = len(shapes)
    rc = lib.pnr_pyramid_to_latent(_ptrs([FAKE] * n), _ints([s[0] for s in shapes]), _ints([s[1] for s in shapes]),
                                   _ints([s[2] for s in shapes]), n, NV, FAKE, None, None)
    return rc, lib.pnr_last_error()


def test_declared_exported_bound_and_revision_still_12(lib, repo_root):
    src = open(os.path.join(repo_root, "include", "pixelnerf_hip.h")).read()
    assert int(re.search(r"#define\s+PNR_ABI_VERSION\s+(\d+)", src).group(1)) == 12 == _lib.ABI_VERSION == lib.pnr_abi_version()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", code)
    assert decl, "not declared in include/pixelnerf_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 9 and args[0].startswith("const float *") and args[1].startswith("int ") and args[-1].startswith("void *")
    comment = src[:src.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "encoder.py:150-163" in comment and "autograd" in comment
    assert hasattr(lib, NAME)
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 9


def test_null_and_invalid_arguments(lib):
    ok = [(64, 8, 8), (128, 4, 4)]
    rc, err = backward(lib, [(64, 4, 4)] * 6, 1)  # 6 stages
    assert rc == -1 and b"1..5 stages" in err and err.startswith(NAME.encode())
    assert lib.pnr_pyramid_to_latent_backward(FAKE, 0, _ptrs([FAKE]), _ints([64]), _ints([4]), _ints([4]), 0, 1, None) == -1  # 0 stages
    assert b"1..5 stages" in lib.pnr_last_error()
    rc, err = backward(lib, ok, 1, d_latent=None)
    assert rc == -1 and b"null argument" in err
    assert lib.pnr_pyramid_to_latent_backward(FAKE, 0, None, _ints([64]), _ints([4]), _ints([4]), 1, 1, None) == -1
    assert lib.pnr_pyramid_to_latent_backward(FAKE, 0, _ptrs([FAKE]), None, _ints([4]), _ints([4]), 1, 1, None) == -1
    assert lib.pnr_pyramid_to_latent_backward(FAKE, 0, _ptrs([FAKE]), _ints([64]), None, _ints([4]), 1, 1, None) == -1
    assert lib.pnr_pyramid_to_latent_backward(FAKE, 0, _ptrs([FAKE]), _ints([64]), _ints([4]), None, 1, 1, None) == -1
    rc, err = backward(lib, ok, 1, stage_ptrs=[FAKE, None])  # a null stage pointer
    assert rc == -1 and b"multiples of 64" in err
    for bad in ([(96, 8, 8)], [(64, 8, 8), (0, 4, 4)], [(64, 0, 8)], [(64, 8, -1)], [(-64, 8, 8)]):
        rc, err = backward(lib, bad, 1)
        assert rc == -1 and b"multiples of 64" in err, bad
    rc, err = backward(lib, ok, -1)
    assert rc == -1 and b"bad sizes" in err
    rc, err = backward(lib, ok, 1, d_latent=FAKE + 4)  # the kernel reads 16 bytes per lane
    assert rc == -1 and b"16-byte aligned" in err


# every size limit of the forward, with the word its message carries
REJECTED = [
    ([(64, 4096, 2048)], 1, b"below 2 GiB"),                       # C H W of one view >= 2^29
    ([(8192, 8, 8)], 1, b"do not fit the LDS"),                    # source windows of the shortest run beyond 160 KiB
    ([(64, 4, 8), (64, 4, 290)], 1, b"32x wider"),                 # a stage far wider than stage 0 (windows still fit)
    ([(64, 65536, 1)], 1, b"grid too large"),                      # H0 beyond the grid's y extent
    ([(64, 8, 8)], 65536, b"grid too large"),                      # NV beyond the grid's z extent
]


@pytest.mark.parametrize("shapes,NV,word", REJECTED, ids=[w.decode().replace(" ", "_") + str(i) for i, (_, _, w) in enumerate(REJECTED)])
@pytest.mark.parametrize("nchw", [0, 1])
def test_rejects_what_the_forward_rejects(lib, shapes, NV, word, nchw):
    rc_f, err_f = forward(lib, shapes, NV)
    assert rc_f == -1 and word in err_f and err_f.startswith(b"pnr_pyramid_to_latent:")
    rc_b, err_b = backward(lib, shapes, NV, nchw=nchw)
    assert rc_b == -1 and word in err_b and err_b.startswith(NAME.encode() + b":")
    assert err_b.split(b": ", 1)[1] == err_f.split(b": ", 1)[1]


def test_no_views_is_ok_without_a_launch(lib):
    for shapes in ([(64, 8, 8)], [(64, 150, 200), (64, 150, 200), (128, 75, 100), (256, 38, 50)], [(64, 65536, 1)]):
        for nchw in (0, 1):
            rc, _ = backward(lib, shapes, 0, nchw=nchw)
            assert rc == 0
    rc, _ = forward(lib, [(64, 8, 8)], 0)
    assert rc == 0


def test_ops_wrapper_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from pixelnerf_amd import ops
    with pytest.raises(_lib.PixelNerfHipError, match="HIP device"):
        ops.pyramid_to_latent_backward(torch.zeros(1, 4, 4, 128), [(1, 64, 4, 4), (1, 64, 2, 2)])
    with pytest.raises(ValueError):
        ops.pyramid_to_latent_backward(torch.zeros(1, 4, 4, 128), [])
    with pytest.raises(ValueError):
        ops.pyramid_to_latent_backward(torch.zeros(1, 4, 4, 128), [(1, 64, 4, 4), (2, 64, 2, 2)])
