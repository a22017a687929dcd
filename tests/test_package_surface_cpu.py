"""The package's surface after its split into submodules, held against tests/golden/package_surface.json -- the record that
tests/golden/make_package_surface.py made from the one-file package before the split: every name, signature, docstring, constant and
SIGNATURES entry is as it was, importing stays lazy, and the argument checks refuse with the messages they always had before
anything touches a device.  Needs neither the library nor a GPU."""
import glob
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import svoslam_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_package_surface as record_maker  # noqa: E402

pkg = svoslam_pkg.load()
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "package_surface.json")))
NOW = record_maker.surface(pkg)


def test_every_recorded_name_is_present_and_identical():
    missing = sorted(set(RECORD["attributes"]) - set(NOW["attributes"]))
    assert not missing, "names the package no longer binds: %s" % missing
    changed = sorted(n for n, was in RECORD["attributes"].items() if NOW["attributes"][n] != was)
    assert not changed, "names bound to something else than before: %s" % changed
    for name in record_maker.PRIVATE:
        assert name in RECORD["attributes"], name


def test_no_public_name_beyond_the_record():
    public = sorted(n for n, v in vars(pkg).items() if not n.startswith("_") and not isinstance(v, types.ModuleType))
    extra = [n for n in public if n not in RECORD["attributes"] and n != "SIGNATURES"]
    assert not extra, "new public names: %s" % extra


def test_signatures_is_one_dict_with_the_same_entries():
    assert isinstance(pkg.SIGNATURES, dict)
    assert list(NOW["signatures"]) == list(RECORD["signatures"])
    assert NOW["signatures"] == RECORD["signatures"]


def test_importing_the_package_loads_neither_torch_nor_the_library():
    code = ("import sys; sys.path.insert(0, %r); import svoslam_pkg; pkg = svoslam_pkg.load(); abi = sys.modules['octree_slam_amd._abi'];"
            "assert 'torch' not in sys.modules, 'torch was imported'; assert abi._lib is None and abi._raw_stream is None and abi._hiplib is None;"
            "assert not hasattr(pkg, '_lib'), 'the handle is cached in _abi alone'; print('lazy')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "lazy", out.stderr


O2, O3, D3 = (0, 0), (0, 0, 0), (2, 2, 2)
REGION_CALLS = {    # every wrapper that takes a region, as a call of (origin, dims); nothing else of it is reached
    "distance_field": lambda o, n: pkg.distance_field(None, None, 5, o, n, 1),
    "reach_field": lambda o, n: pkg.reach_field(None, None, 5, o, n, 0, []),
    "owner_field": lambda o, n: pkg.owner_field(None, None, 5, o, n, 0, seeds=[]),
    "cost_field": lambda o, n: pkg.cost_field(None, None, 5, o, n, 0, 0, None, []),
    "ground_field": lambda o, n: pkg.ground_field(None, None, 5, o, n, "+y", 0, 2, 1, 0, []),
    "label_components": lambda o, n: pkg.label_components(None, None, 5, o, n, 0),
    "nearest_field": lambda o, n: pkg.nearest_field(None, None, 5, o, n, 1),
    "visibility_field": lambda o, n: pkg.visibility_field(None, None, 5, o, n, 4, []),
    "cover_views": lambda o, n: pkg.cover_views(None, None, 5, o, n, 4, [], 1),
    "observe_rays": lambda o, n: pkg.observe_rays(None, None, 5, (0, 0, 0), 1.0, o, n, [], []),
    "frontier_field": lambda o, n: pkg.frontier_field(None, None, 5, o, n, []),
    "score_poses": lambda o, n: pkg.score_poses(None, [], 5, (0, 0, 0), 1.0, o, n, [], [], 1),
    "trace_paths": lambda o, n: pkg.trace_paths([], o, n, [], 0),
    "segment_clearance": lambda o, n: pkg.segment_clearance([], o, n, []),
    "shorten_paths": lambda o, n: pkg.shorten_paths([], o, n, 0, [], []),
    "trace_ground_paths": lambda o, n: pkg.trace_ground_paths([], o, n, "+y", 1, 0, [], 0),
}


@pytest.mark.parametrize("name", sorted(REGION_CALLS))
def test_a_two_element_origin_or_dims_is_refused(name):
    for origin, dims in ((O2, D3), (O3, (2, 2))):
        with pytest.raises(ValueError) as e:
            REGION_CALLS[name](origin, dims)
        assert str(e.value) == "origin and dims are three cells each (x, y, z)"


def test_a_host_or_wrongly_typed_tensor_is_refused_by_name():
    host = torch.zeros((2, 3), dtype=torch.int32)
    wide = torch.zeros((2, 3), dtype=torch.int64)
    calls = {
        # (owner_field allocates its outputs before it looks at the seeds: tests/test_gpu_arg_forms.py has it)
        "seeds": [lambda t: pkg.reach_field(None, None, 5, O3, D3, 0, t), lambda t: pkg.cost_field(None, None, 5, O3, D3, 0, 0, None, t),
                  lambda t: pkg.ground_field(None, None, 5, O3, D3, "+y", 0, 2, 1, 0, t)],
        "views": [lambda t: pkg.visibility_field(None, None, 5, O3, D3, 4, t)],
        "candidates": [lambda t: pkg.cover_views(None, None, 5, O3, D3, 4, t, 1)],
        "field": [lambda t: pkg.score_poses(None, t, 5, (0, 0, 0), 1.0, O3, D3, [], [], 1)],
    }
    for what, fns in calls.items():
        for fn in fns:
            for t in (host, wide):
                with pytest.raises(ValueError) as e:
                    fn(t)
                assert str(e.value) == "a %s tensor is int32 on the device" % what


def test_an_unknown_output_is_refused_with_the_outputs_there_are():
    # a KeyError, as it always was: the wrappers look the name up among their outputs
    calls = {
        "dist2, cell, node, color": lambda w: pkg.nearest_field(None, None, 5, O3, D3, 1, want=w),
        "mask, count": lambda w: pkg.visibility_field(None, None, 5, O3, D3, 4, [], want=w),
        "seen, chosen, gain, round, summary": lambda w: pkg.cover_views(None, None, 5, O3, D3, 4, [], 1, want=w),
        "state, frontier, summary": lambda w: pkg.frontier_field(None, None, 5, O3, D3, [], want=w),
        "cost, near, far, outside, best": lambda w: pkg.score_poses(None, [], 5, (0, 0, 0), 1.0, O3, D3, [], [], 1, want=w),
    }
    for have, fn in calls.items():
        with pytest.raises(KeyError) as e:
            fn(("nope",))
        assert e.value.args[0] == "no output 'nope' (have: %s)" % have


def test_each_shared_message_has_one_home_and_no_module_is_long():
    sources = {p: open(p).read() for p in glob.glob(os.path.join(svoslam_pkg.PKG_DIR, "*.py"))}
    for text in ("origin and dims are three cells each", "tensor is int32 on the device", "no output %r"):
        assert sum(s.count(text) for s in sources.values()) == 1, text
    lines = {os.path.basename(p): s.count("\n") for p, s in sources.items()}
    assert lines["__init__.py"] < 100
    split = {n: k for n, k in lines.items() if n.startswith("_") and n != "__init__.py"}
    assert len(split) >= 10 and max(split.values()) <= 700, split
