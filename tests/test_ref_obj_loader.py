"""Pins the OBJ loading half of the mesh path (SURVEY.md 8a row a12's input side) against the REFERENCE's
own loader: tests/golden/ref_obj_loader.json holds digests of what the reference's objUtil code (compiled
from the reference's sources by `make -C oracle ref`, run by tests/golden/make_ref_obj_golden.py) produces; the
oracle's restatement (ora_mesh_load_obj) and the product's host loader (svoslam_mesh_load_obj) must
reproduce them bit for bit.  The reference's OBJ files are committed as data fixtures (tests/golden/ref_objs.npz,
tests/data/), the reference loader's arrays for the generated files as tests/golden/ref_obj_loader_arrays.npz."""
import hashlib
import json
import os
import sys

import numpy as np

import meshgen

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_ref_obj_golden import digest  # noqa: E402
from util import reference_obj  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "ref_obj_loader.json")))
REF_ARRAYS = os.path.join(HERE, "golden", "ref_obj_loader_arrays.npz")     # the reference loader's output on meshgen's files


def product_mesh(path):
    import svoslam_pkg
    m = svoslam_pkg.load().Mesh(str(path))
    b0, b1 = m.bbox()
    return {"vbo": m.vbo(), "tbo": m.tbo(), "bbox0": b0, "bbox1": b1}


def strip(rec):
    return {k: v for k, v in rec.items() if k != "input_sha256"}


def test_generated_objs_match_reference_loader(tmp_path, oracle):
    paths = meshgen.write_generated_objs(str(tmp_path))
    assert sorted(paths) == sorted(GOLDEN["generated"])
    for name, path in sorted(paths.items()):
        want = strip(GOLDEN["generated"][name])
        assert digest(oracle.mesh_load_obj(path)) == want, "oracle loader differs from the reference on " + name
        assert digest(product_mesh(path)) == want, "product loader differs from the reference on " + name


def test_reference_objs_match_reference_loader(tmp_path, oracle):
    for name, rec in sorted(GOLDEN["reference_objs"].items()):
        path = reference_obj(name, tmp_path)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == rec["input_sha256"], name   # the file the digests were made from
        assert digest(oracle.mesh_load_obj(path)) == strip(rec), name
        assert digest(product_mesh(path)) == strip(rec), name


def recorded_reference_load(arrays, name):
    return {"vbo": arrays[name + "/vbo"], "tbo": arrays[name + "/tbo"] if name + "/tbo" in arrays else None,
            "bbox0": arrays[name + "/bbox0"], "bbox1": arrays[name + "/bbox1"]}


def test_live_reference_loader(tmp_path, oracle):
    """the reference loader itself, array against array (not only digests): its recorded output on the generated files, and
    where the reference's sources are at hand (`make -C oracle ref`), the compiled loader run live as well"""
    import numpy as np
    arrays = dict(np.load(REF_ARRAYS))
    live = oracle.reference_obj_available()            # (build() compiles it where the reference is present)
    paths = meshgen.write_generated_objs(str(tmp_path))
    for name, path in sorted(paths.items()):
        rec = recorded_reference_load(arrays, name)
        assert digest(rec) == strip(GOLDEN["generated"][name]), name      # the recorded arrays are those the digests pin
        refs = [rec, oracle.reference_obj_load(path)] if live else [rec]
        for ref in refs:
            check_same_arrays(ref, oracle.mesh_load_obj(path), name)


def check_same_arrays(ref, mine, name):
    import numpy as np
    assert ref["vbo"].shape == mine["vbo"].shape, name
    assert np.array_equal(ref["vbo"].view(np.uint32), mine["vbo"].view(np.uint32)), name
    assert (ref["tbo"] is None) == (mine["tbo"] is None), name
    if ref["tbo"] is not None:
        assert np.array_equal(ref["tbo"].view(np.uint32), mine["tbo"].view(np.uint32)), name
    assert np.array_equal(ref["bbox0"], mine["bbox0"]) and np.array_equal(ref["bbox1"], mine["bbox1"]), name
