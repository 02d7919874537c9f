"""The typed native-call layer, without a GPU: the prototype table is what the header says, the typed handle rejects
a wrong call before the library is entered, and every call site of the package passes plain values in the header's
number."""
import ast
import ctypes
import importlib.util
import os

import pytest
import torch

from test_capi_and_host import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-splatting-toolkit_amd")


def _generator():
    spec = importlib.util.spec_from_file_location("gen_prototypes", os.path.join(ROOT, "tools", "gen_prototypes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_table_is_what_the_generator_writes():
    from rasterizer.cuda import _backend
    from rasterizer.cuda._prototypes import PROTOTYPES

    gen = _generator()
    with open(gen.OUTPUT) as f:
        assert f.read() == gen.generate(), "rasterizer/cuda/_prototypes.py is stale: run tools/gen_prototypes.py"
    assert sorted(PROTOTYPES) == header_symbols()
    assert _backend.SYMBOLS == tuple(PROTOTYPES)
    assert [n for n, _, _ in gen.parse(open(gen.HEADER).read())] == list(PROTOTYPES)  # header order
    for name, (ret, params) in PROTOTYPES.items():
        assert ret in "izqs", name  # int, size_t, long long, const char *
        assert set(params) <= set("piIfdzqQ"), name
    assert PROTOTYPES["gsr_last_error"] == ("s", "") and PROTOTYPES["gsr_calibrate_valu"][0] == "q"
    assert PROTOTYPES["gsr_sort_workspace_bytes"] == ("z", "i")
    assert PROTOTYPES["gsr_project_forward"] == ("i", "ippfpppffffIIIfpppppppp")


def test_generator_skips_defines_comments_and_struct_bodies():
    gen = _generator()
    text = """
    #define GSR_A (1 << 30) /* gsr_not_an_entry(int) */
    #define GSR_B(k) \\
        (((k) & 63) << 22)
    typedef void *gsr_stream_t;
    typedef struct gsr_desc { int n; const float *p; } gsr_desc;
    // gsr_neither(int x);
    #define GSR_C 4
    size_t gsr_bytes(int n, unsigned int m);
    const char *gsr_text(void);
    int gsr_run(const gsr_desc *d, const float *x, float *y, unsigned long long seed, long long n, double b,
                size_t bytes, gsr_stream_t stream);
    """
    assert gen.parse(text) == [("gsr_bytes", "z", "iI"), ("gsr_text", "s", ""), ("gsr_run", "i", "pppQqdzp")]
    with pytest.raises(ValueError):
        gen.parse("int gsr_by_value(gsr_desc d);")


_PROJECT_FORWARD = (4, None, None, 1.0, None, None, None, 1.0, 1, 0.0, 0.0, 8, 8, 17, 0.01,
                    None, None, None, None, None, None, None, None)


def test_typed_handle_checks_count_and_kind_before_the_library():
    """Entries that reject on the host before they touch a device (as test_argument_validation_needs_no_gpu)."""
    from rasterizer.cuda import _backend, _call

    args = list(_PROJECT_FORWARD)
    args[1] = torch.zeros((4, 3))  # means3d: a CPU tensor converts like any other
    with pytest.raises(RuntimeError, match="block_width"):
        _call("gsr_project_forward", *args)
    with pytest.raises(TypeError):
        _call("gsr_project_forward", *args[:-1])
    with pytest.raises(ctypes.ArgumentError):
        _call("gsr_project_forward", "4", *args[1:])  # a str for num_points
    with pytest.raises(ctypes.ArgumentError):
        _call("gsr_project_forward", 4, 1.5, *args[2:])  # a float for a pointer
    with pytest.raises(ctypes.ArgumentError):
        _call("gsr_project_forward", 4, "means3d", *args[2:])  # c_void_p alone would take a str's characters
    with pytest.raises(ctypes.ArgumentError):
        _call("gsr_project_forward", 4.0, *args[1:])  # a float for an int

    T = _backend.typed()
    assert T.gsr_sort_workspace_bytes(0) == 0  # size_t return
    assert T.gsr_version() == 200
    assert T.gsr_last_error.restype is ctypes.c_char_p
    # what call sites and tests wrap by hand passes unchanged: the parameter's own type, c_void_p, byref, arrays
    desc = (ctypes.c_int * 4)()
    wrapped = [ctypes.c_int(4), ctypes.c_void_p(args[1].data_ptr()), ctypes.byref(desc), ctypes.c_float(1.0), desc,
               args[1].data_ptr()] + args[6:]
    with pytest.raises(RuntimeError, match="block_width"):
        _call("gsr_project_forward", *wrapped)

    # the raw handle is untouched: return types only, its own function objects
    L = _backend.lib()
    assert L is not T and L.gsr_project_forward is not T.gsr_project_forward
    for name in _backend.SYMBOLS:
        assert getattr(L, name).argtypes is None, name
    assert len(T.gsr_project_forward.argtypes) == 23
    assert L.gsr_sort_workspace_bytes.restype is ctypes.c_size_t and L.gsr_last_error.restype is ctypes.c_char_p
    c_f, c_u = ctypes.c_float, ctypes.c_uint
    assert L.gsr_sh_forward(c_u(4), c_u(5), c_u(0), None, None, None, None) == -1
    assert b"degree" in L.gsr_last_error()
    assert L.gsr_project_forward(ctypes.c_int(4), None, None, c_f(1), None, None, None, c_f(1), c_f(1), c_f(0), c_f(0),
                                 c_u(8), c_u(8), c_u(17), c_f(0.01), None, None, None, None, None, None, None, None) == -1
    assert b"block_width" in T.gsr_last_error()  # one library, one thread-local message


_SCALAR_WRAPPERS = {"c_int", "c_uint", "c_float", "c_size_t", "c_longlong", "c_ulonglong", "c_double"}


def _native_calls(tree):
    """-> [(entry names, argument nodes, lineno)] of the `_call("gsr_x", ...)` and `handle.gsr_x(...)` sites."""
    out = []
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        f = node.func
        if isinstance(f, ast.Name) and f.id == "_call" and node.args:
            first = node.args[0]
            names = [c.value for c in ([first.body, first.orelse] if isinstance(first, ast.IfExp) else [first])
                     if isinstance(c, ast.Constant) and isinstance(c.value, str)]
            assert names, f"line {node.lineno}: _call's entry name is not a literal"
            out.append((names, node.args[1:], node.lineno))
        elif isinstance(f, ast.Attribute) and f.attr.startswith("gsr_") and f.attr != "gsr_last_error":
            out.append(([f.attr], node.args, node.lineno))
    return out


def test_call_sites_pass_plain_values_in_the_headers_number():
    from rasterizer.cuda._prototypes import PROTOTYPES

    sites = counted = 0
    for sub in ("rasterizer", "gs_fused", "gs_fusion", "gs_io", "harness"):
        for dirpath, _, files in os.walk(os.path.join(PKG, sub)):
            for fn in sorted(files):
                if not fn.endswith(".py"):
                    continue
                path = os.path.join(dirpath, fn)
                with open(path) as f:
                    tree = ast.parse(f.read())
                for names, args, line in _native_calls(tree):
                    where = f"{os.path.relpath(path, PKG)}:{line} {'/'.join(names)}"
                    sites += 1
                    for a in args:
                        for n in ast.walk(a):
                            if isinstance(n, ast.Call):
                                callee = n.func.attr if isinstance(n.func, ast.Attribute) else getattr(n.func, "id", "")
                                assert callee not in _SCALAR_WRAPPERS, f"{where}: hand-wrapped scalar {callee}(...)"
                    for name in names:
                        assert name in PROTOTYPES, f"{where}: not an entry of the header"
                    if not any(isinstance(a, ast.Starred) for a in args):
                        counted += 1
                        for name in names:
                            assert len(args) == len(PROTOTYPES[name][1]), \
                                f"{where}: {len(args)} arguments, the header declares {len(PROTOTYPES[name][1])}"
    # (the scan is not vacuous: the package has 128 such sites, 116 of them without a starred argument)
    assert sites >= 120 and counted >= 110, (sites, counted)
