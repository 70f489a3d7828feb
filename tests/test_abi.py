"""CPU: the C-ABI library loads and exports every symbol include/openeat_hip.h
declares, and the ctypes structures have the layout of its structs (no compute is launched here)."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "openeat_hip.h")
LIB = os.path.join(ROOT, "openeat_amd", "lib", "libopeneat_hip.so")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(oe_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(LIB)
    names = declared_functions()
    assert len(names) >= 8
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/openeat_hip.h but not exported"


def test_python_binding_covers_the_header():
    from openeat_amd import hip
    assert sorted(hip.exported_symbols()) == declared_functions()
    lib = hip.lib()
    assert lib.oe_abi_version() >= 1


def test_ctypes_structures_have_the_layout_the_header_declares(tmp_path):
    """Every ctypes.Structure of hip.py against its C struct: a generated host program prints sizeof and the offsetof of every
    field named in _fields_.  The C struct of a class is the one whose name, without oe_ and underscores, is the class name in
    lower case (GemmArgs: oe_gemm_args); the field names are the same on both sides."""
    from openeat_amd import hip
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    c_names = {n[3:].replace("_", ""): n for n in re.findall(r"\btypedef\s+struct\s+(oe_[a-z0-9_]+)\s*\{", src)}
    classes = {name.lower(): cls for name, cls in vars(hip).items() if isinstance(cls, type) and issubclass(cls, ctypes.Structure)
               and cls is not ctypes.Structure}
    assert sorted(classes) == sorted(c_names) and len(classes) >= 11, (sorted(classes), sorted(c_names))
    for new in ("oe_ngram_model", "oe_context_graph", "oe_prefix_beam_args"):
        assert new in c_names.values()
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {"]
    want = {}
    for key, cls in classes.items():
        c = c_names[key]
        lines.append(f'    printf("{c} %zu\\n", sizeof({c}));')
        want[c] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            lines.append(f'    printf("{c}.{field} %zu\\n", offsetof({c}, {field}));')
            want[f"{c}.{field}"] = getattr(cls, field).offset
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.cpp").write_text("\n".join(lines) + "\n")
    subprocess.check_call(["g++", "-std=c++17", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.cpp")])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())}
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
    print(f"{len(classes)} structs, {len(want)} sizes and offsets agree: {', '.join(sorted(c_names.values()))}")


def test_ctc_workspace_covers_both_state_widths():
    """oe_ctc_loss_fused keeps alpha / beta / ll in float32 for launches of T <= 248 frames (the bench's length; the size
    every earlier caller allocated) and in float64 above (include/openeat_hip.h): there the workspace holds lp in float32,
    the label chains, and ll and two trellises as 8-byte aligned doubles."""
    lib = ctypes.CDLL(LIB)
    lib.oe_ctc_workspace_floats.restype = ctypes.c_size_t
    lib.oe_ctc_workspace_floats.argtypes = [ctypes.c_int] * 3
    for B, T, Lmax in ((32, 248, 40), (1, 1, 0), (3, 131, 255)):
        Sp = 2 * Lmax + 1
        assert lib.oe_ctc_workspace_floats(B, T, Lmax) == B + 3 * B * T * Sp + B * Sp + 16
    for B, T, Lmax in ((2, 249, 7), (2, 1500, 200), (1, 2000, 255)):
        Sp = 2 * Lmax + 1
        need = B + B * T * Sp + B * Sp + 1 + 2 * (B + 2 * B * T * Sp + 2)
        assert lib.oe_ctc_workspace_floats(B, T, Lmax) >= need


def test_invalid_arguments_are_reported_not_launched():
    from openeat_amd import hip
    lib = hip.lib()
    rc = lib.oe_layernorm_fwd(None, None, None, 1e-5, 4, 32, None, 0, None, None, None)
    assert rc != 0 and b"null" in lib.oe_last_error()
