"""Regenerates tests/golden/package_surface.json: what the loaded package octree_slam_amd shows its callers, one line an entry.

For every attribute of the package that is no module and no dunder -- the public names, and the private names that tests and
tools reach through the package (PRIVATE) -- the record holds one string: the kind (function, class or constant),
str(inspect.signature) where there is one, the first 16 hex digits of the SHA-256 of __doc__, the value of a plain constant, the
_fields_ of a ctypes structure; and the same for every public or special function and property a class defines itself, under
"Class.member".  For SIGNATURES it holds every symbol as "restype(argtypes)" by type name, in the table's order.

tests/test_package_surface_cpu.py holds the package against the record, so the record is made from the commit BEFORE a change
to the package's layout, never from the changed code:

  python tests/golden/make_package_surface.py      (from the repository root; needs neither the library nor a device)
"""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "package_surface.json")

# the private names that tests and tools reach through the package; every other name with a leading underscore is the binding's
# own business (its helpers, and the library handles it caches)
PRIVATE = ("_ptr", "_fa", "_stream", "_hip", "_PoolStruct", "_ReachStats", "_OwnerStats", "_PlanStats", "_GroundStats", "_ComponentStats")


def type_name(t):
    """a ctypes type by name: c_int, LP_c_float, c_int_Array_3, _PoolStruct, ...; None stays None"""
    return "None" if t is None else t.__name__


def doc_digest(obj):
    doc = getattr(obj, "__doc__", None)
    return "doc:none" if doc is None else "doc:" + hashlib.sha256(doc.encode()).hexdigest()[:16]


def signature(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return "(?)"


def describe(name, obj, out):
    """the entry of `obj` into out[name]; a class also enters its members as out["name.member"]"""
    if isinstance(obj, types.FunctionType):
        out[name] = "function %s %s" % (signature(obj), doc_digest(obj))
    elif isinstance(obj, property):
        out[name] = "property %s" % doc_digest(obj)
    elif isinstance(obj, type):
        out[name] = "class %s %s bases %s" % (signature(obj), doc_digest(obj), ",".join(b.__name__ for b in obj.__bases__))
        if issubclass(obj, C.Structure):
            out[name] += " fields " + ",".join("%s:%s" % (f[0], type_name(f[1])) for f in obj._fields_)
        for member, value in sorted(vars(obj).items()):
            if isinstance(value, (types.FunctionType, property)) and (not member.startswith("_") or member.startswith("__")):
                describe("%s.%s" % (name, member), value, out)
    else:
        if isinstance(obj, str) and os.path.isabs(obj):               # LIB_PATH, HEADER_PATH: wherever the repository lies
            obj = "<root>/" + os.path.relpath(obj, ROOT).replace(os.sep, "/")
        out[name] = "constant %s %s" % (type(obj).__name__, json.dumps(obj))


def surface(pkg):
    """the record of a loaded package"""
    names = sorted(n for n, v in vars(pkg).items() if not isinstance(v, types.ModuleType) and not n.startswith("__")
                   and (not n.startswith("_") or n in PRIVATE) and n != "SIGNATURES")
    attributes = {}
    for n in names:
        describe(n, getattr(pkg, n), attributes)
    symbols = {n: "%s(%s)" % (type_name(res), ", ".join(type_name(a) for a in args)) for n, (res, args) in pkg.SIGNATURES.items()}
    return {"attributes": attributes, "signatures": symbols}


if __name__ == "__main__":
    import svoslam_pkg
    record = surface(svoslam_pkg.load())
    json.dump(record, open(OUT, "w"), indent=0)
    print("wrote", OUT, "-- %d entries, %d symbols" % (len(record["attributes"]), len(record["signatures"])))
