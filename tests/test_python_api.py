"""The public surface of query, shade and path is pinned: tests/golden/python_api.json holds, for every public function, its
signature and the SHA-256 of its docstring (through inspect.cleandoc, so that the interpreter's own stripping of a docstring's
indentation, which came with Python 3.13, changes nothing), and for every named tuple its fields, as they were before the wrappers moved onto
query._OnStream.  A change of a name, a parameter, a default or a docstring shows here.  The file is the output of

    import json, sys; sys.path[:0] = [".", "tests"]; from test_python_api import surface
    json.dump(surface(), open("python_api.json", "w"), indent=1, sort_keys=True)

run at the root of a checkout of the commit whose surface is to be kept, with this file copied into its tests/."""
import hashlib
import inspect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_api.json")


def surface():
    from ezrt_amd import path, query, shade
    api = {}
    for mod in (query, shade, path):
        short = mod.__name__.rsplit(".", 1)[-1]
        for name, x in sorted(vars(mod).items()):
            if name.startswith("_") or getattr(x, "__module__", None) != mod.__name__:
                continue
            if inspect.isfunction(x):
                api["%s.%s" % (short, name)] = {"signature": str(inspect.signature(x)),
                                                "doc_sha256": hashlib.sha256(inspect.cleandoc(x.__doc__ or "").encode()).hexdigest()}
            elif isinstance(x, type) and issubclass(x, tuple) and hasattr(x, "_fields"):
                api["%s.%s" % (short, name)] = {"fields": list(x._fields)}
    return api


def test_public_surface_is_the_golden_one():
    with open(GOLDEN) as f:
        golden = json.load(f)
    now = surface()
    assert sorted(now) == sorted(golden)
    for name in golden:
        assert now[name] == golden[name], name
    # what the file is expected to cover: query's functions and named tuples, shade's five and path's two functions
    assert sum(1 for k, v in golden.items() if k.startswith("query.") and "signature" in v) == 58
    assert sum(1 for k, v in golden.items() if k.startswith("shade.") and "signature" in v) == 5
    assert sum(1 for k, v in golden.items() if k.startswith("path.") and "signature" in v) == 2
