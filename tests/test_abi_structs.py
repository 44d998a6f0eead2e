"""CPU tier of the row-table wrappers' shared layer (picasso_amd/backend.py): the ctypes structures, the ``_AREAS_GEOM``
dtype and the constants that restate include/picasso_hip.h equal what the host C compiler makes of that header, field
by field; and the TypeError / ValueError texts of the dtype and length checks are pinned as literals, every accepted
dtype and every refused one, each wording at the call site that raises it.  The uploads are replaced by host tensors:
no check here needs a device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from picasso_amd import _lib, backend

STRUCTS = {"pmi_link_column": backend._LinkColumn, "pmi_centers_column": backend._CentersColumn,
           "pmi_kinetics_column": backend._KineticsColumn, "pmi_combine_column": backend._CombineColumn,
           "pmi_knn_grid": backend._KnnGrid, "pmi_areas_columns": backend._AreasColumns}
CONSTANTS = {"PMI_LINK_F32": backend.LINK_F32, "PMI_LINK_F64": backend.LINK_F64, "PMI_LINK_U32": backend.LINK_U32,
             "PMI_LINK_U64": backend.LINK_U64, "PMI_LINK_SUM": backend.LINK_SUM, "PMI_LINK_WSUM": backend.LINK_WSUM,
             "PMI_LINK_XWSUM": backend.LINK_XWSUM,
             "PMI_CENTERS_F32": backend.centers_type(np.float32), "PMI_CENTERS_F64": backend.centers_type(np.float64),
             "PMI_CENTERS_U32": backend.centers_type(np.uint32), "PMI_CENTERS_I32": backend.centers_type(np.int32),
             "PMI_CENTERS_U64": backend.centers_type(np.uint64), "PMI_CENTERS_I64": backend.centers_type(np.int64),
             "PMI_CENTERS_MEAN": backend.CENTERS_MEAN, "PMI_CENTERS_XSUM": backend.CENTERS_XSUM,
             "PMI_CENTERS_FIRST": backend.CENTERS_FIRST, "PMI_CENTERS_EVENTS": backend.CENTERS_EVENTS,
             "PMI_AREAS_LDS_BINS": backend.AREAS_LDS_BINS, "PMI_AREAS_MAX_BINS": backend.AREAS_MAX_BINS}
SIZES = {"pmi_link_column": 40, "pmi_centers_column": 56, "pmi_kinetics_column": 32, "pmi_combine_column": 56,
         "pmi_knn_grid": 40, "pmi_areas_columns": 56, "pmi_areas_geom": 72}      # what the header gave when this was written


def python_layout():
    """{"sizeof S": n, "S.field": offset, "CONSTANT": value} as backend.py states them."""
    out = dict(CONSTANTS)
    for name, struct in STRUCTS.items():
        out["sizeof " + name] = ctypes.sizeof(struct)
        for field, _ in struct._fields_:
            out[name + "." + field] = getattr(struct, field).offset
    out["sizeof pmi_areas_geom"] = backend._AREAS_GEOM.itemsize
    for field in backend._AREAS_GEOM.names:
        out["pmi_areas_geom." + field] = backend._AREAS_GEOM.fields[field][1]
    return out


@pytest.fixture(scope="module")
def header_layout(tmp_path_factory):
    """The same keys from a C99 program compiled against the header with the host compiler."""
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    lines = []
    for key in python_layout():
        if key.startswith("sizeof "):
            lines.append(f'printf("{key} %ld\\n", (long)sizeof({key[7:]}));')
        elif "." in key:
            struct, field = key.split(".")
            lines.append(f'printf("{key} %ld\\n", (long)offsetof({struct}, {field}));')
        else:
            lines.append(f'printf("{key} %ld\\n", (long)({key}));')
    tmp = tmp_path_factory.mktemp("abi")
    src, exe = tmp / "layout.c", tmp / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "picasso_hip.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in text.splitlines()}


def test_structures_and_constants_equal_the_header(header_layout):
    ours = python_layout()
    assert set(header_layout) == set(ours)
    assert {k: (header_layout[k], v) for k, v in ours.items() if header_layout[k] != v} == {}
    assert {name: header_layout["sizeof " + name] for name in SIZES} == SIZES


# ---- the dtype checks ----------------------------------------------------------------------------------------------
LINK_CODES = {"float32": 0, "float64": 1, "uint32": 2, "int32": 2, "uint64": 3, "int64": 3}
CENTERS_CODES = {"float32": 0, "float64": 1, "uint32": 2, "int32": 3, "uint64": 4, "int64": 5}
REFUSED = ("float16", "complex64", "complex128", "bool", "int8", "uint8", "int16", "uint16")


@pytest.mark.parametrize("fn,codes,what", [(backend.link_type, LINK_CODES, "link / NeNA"),
                                           (backend.centers_type, CENTERS_CODES, "the cluster centers")])
def test_type_codes(fn, codes, what):
    import torch
    for name, code in codes.items():
        assert fn(np.dtype(name)) == code and fn(getattr(np, name)) == code
        if name[0] == "f":
            assert fn(name, True) == code and fn(getattr(torch, name), True) == code
        else:
            with pytest.raises(TypeError) as e:
                fn(name, True)
            assert str(e.value) == f"unsupported column dtype {name} for {what} on the device"
    for name in REFUSED:
        for floating in (False, True):
            with pytest.raises(TypeError) as e:
                fn(np.dtype(name), floating)
            assert str(e.value) == f"unsupported column dtype {name} for {what} on the device"


def test_index_column():
    for name in ("bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64"):
        got = backend._index_column(np.ones(3, name), "frame")
        assert got.dtype == np.int64 and got.tolist() == [1, 1, 1]
    for name in ("float16", "float32", "float64", "complex64"):
        with pytest.raises(TypeError) as e:
            backend._index_column(np.ones(3, name), "group")
        assert str(e.value) == f"group must be an integer column, not {name}"


def test_centers_column():
    widened = {"bool": "int32", "int8": "int32", "int16": "int32", "uint8": "uint32", "uint16": "uint32"}
    for name in list(CENTERS_CODES) + list(widened):
        got = backend._centers_column(np.ones(3, name), "a statistics column")
        assert got.dtype == np.dtype(widened.get(name, name)) and got.tolist() == [1, 1, 1]
    for name in ("float16", "complex64", "complex128"):
        with pytest.raises(TypeError) as e:
            backend._centers_column(np.ones(3, name), "a statistics column")
        assert str(e.value) == f"unsupported column dtype {name} for the cluster centers on the device"
    with pytest.raises(ValueError) as e:
        backend._centers_column(np.ones((2, 2)), "a statistics column")
    assert str(e.value) == "a statistics column must be a column, not an array of shape (2, 2)"


def test_combine_floats():
    for name in ("float32", "float64"):
        assert backend._combine_floats(np.ones(3, name)[::1], "the weights").dtype == np.dtype(name)
    for name in ("float16", "complex64", "bool", "int32", "int64"):
        with pytest.raises(TypeError) as e:
            backend._combine_floats(np.ones(3, name), "the weights")
        assert str(e.value) == f"the weights must be a float32 or float64 column, not {name} of shape (3,)"
    with pytest.raises(TypeError) as e:
        backend._combine_floats(np.ones((2, 2)), "an averaged column")
    assert str(e.value) == "an averaged column must be a float32 or float64 column, not float64 of shape (2, 2)"


def test_knn_points():
    assert backend.knn_points(np.ones((4, 3), np.float32)).dtype == np.float64
    for bad in (np.ones(4), np.ones((4, 4)), np.ones((2, 2, 2))):
        with pytest.raises(ValueError) as e:
            backend.knn_points(bad)
        assert str(e.value) == f"points must have shape (n, 2) or (n, 3), not {bad.shape}"


# ---- the checks that sit behind an upload: the upload is a host tensor here -----------------------------------------
@pytest.fixture
def host_uploads(monkeypatch):
    import torch

    def to_host_tensor(a, dtype=None):
        a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype, copy=False))
        if a.dtype in (np.uint32, np.uint64):
            a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
        return torch.from_numpy(a)

    monkeypatch.setattr(backend, "_to_device", to_host_tensor)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def test_float_column(host_uploads):
    import torch
    for name, code in (("float32", backend.LINK_F32), ("float64", backend.LINK_F64)):
        t, got = backend._float_column(np.ones(3, name))
        assert got == code and t.dtype == getattr(torch, name)
    for name in ("float16", "complex64", "bool", "int32", "uint32", "int64", "uint64"):
        with pytest.raises(TypeError) as e:
            backend._float_column(np.ones(3, name))
        assert str(e.value) == f"unsupported column dtype {name} for link / NeNA on the device"
    # a tensor that is not on the GPU, not 1-D or not float32 / float64: one wording
    for bad in (torch.ones(3), torch.ones(3, dtype=torch.float16), torch.ones(3, dtype=torch.int64),
                torch.ones((2, 2), dtype=torch.float64)):
        with pytest.raises(TypeError) as e:
            backend._float_column(bad)
        assert str(e.value) == "a device column must be a 1-D float32 or float64 tensor on the GPU"


def test_length_checks(host_uploads):
    per_row = "every column must have one entry per row of the table"
    ones = np.ones(3, np.float32)

    table = backend.BlockTable.__new__(backend.BlockTable)
    table.n = 3
    assert [len(c) for c in table._columns(ones, ones)[::2]] == [3, 3]
    for x, y in ((ones[:2], ones), (ones, np.ones(4))):
        with pytest.raises(ValueError) as e:
            table._columns(x, y)
        assert str(e.value) == "x and y must have one entry per row of the table"

    groups = backend.CombineGroups.__new__(backend.CombineGroups)
    groups.n, groups.n_groups, groups.device = 3, 1, "cpu"
    groups._cache = backend._Uploads(3)
    assert len(groups._dev(ones)) == 3
    for call in (lambda: groups._dev(np.ones(2)), lambda: groups.weights(ones[:2], ones),
                 lambda: groups.weights(ones, np.ones(4)), lambda: backend.combine_stats(groups, moments=[np.ones(4)])):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == per_row
    for x, w in ((ones, np.ones(3)), (ones[:2], ones), (ones, ones[:2])):
        with pytest.raises(ValueError) as e:
            backend.combine_stats(groups, averages=[(x, w)])
        assert str(e.value) == "an averaged column and its weights must have one floating type and one entry per row"

    frame = np.zeros(3, np.int64)
    for args in ((frame[:2], ones, ones, frame), (frame, ones, ones[:2], frame), (frame, ones, ones, frame[:2])):
        with pytest.raises(ValueError) as e:
            backend.LinkTable(*args)
        assert str(e.value) == "frame, x, y and group must have one length"
    with pytest.raises(ValueError) as e:
        backend.picks_square(ones, ones[:2], np.zeros((1, 4)), np.zeros(1, np.uint8))
    assert str(e.value) == "x and y must have one length"
    with pytest.raises(ValueError) as e:
        backend.picks_square(ones, ones, np.zeros((2, 4)), np.zeros(1, np.uint8))
    assert str(e.value) == "one flag byte per pick"
    for fr, col in ((frame, ones[:2]), (frame[:2], ones)):
        with pytest.raises(ValueError) as e:
            backend.fiducials_drift(np.array([0, 3]), fr, [col], 5)
        assert str(e.value) == "frame and the columns must have offsets[-1] rows"
    with pytest.raises(ValueError) as e:
        backend.DarkTable(frame, frame[:2], frame)
    assert str(e.value) == "frame, group and last_frame must have one length, of at least one row"



def test_the_gpu_tier_expectations_need_no_device():
    """What tests/test_gpu_wrappers_shared.py holds the device against is checked here, where every pull request runs it."""
    import test_gpu_wrappers_shared as shared
    shared.check_host_references()
