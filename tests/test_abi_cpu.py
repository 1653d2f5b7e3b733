"""The one place that holds the Python binding to include/qs_amd.h: every prototype against qs_amd.lib.SIGNATURES argument by argument, every
struct with a body against its ctypes mirror in qs_amd.lib.STRUCTS (a C compile of the header gives sizes and offsets), the ABI numbers, and
the Python tables that restate the header's enums.  Only the ABI numbers ask the built library; what it exports and how load() binds it is
test_host_cpu.py's test_library_exports_every_declared_symbol."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from qs_amd import ars, lib, mpc, policy, vec_env

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "qs_amd.h")).read(), flags=re.S)   # (the header has no // comments)

RETURNS = {"void": None, "const char*": C.c_char_p, "int": C.c_int}
C_KINDS = {"int": "int", "int32_t": "int", "float": "float", "double": "double", "long long": "long long", "uint64_t": "u64", "unsigned long long": "u64"}
CTYPES_KINDS = {C.c_int: "int", C.c_int32: "int", C.c_float: "float", C.c_double: "double", C.c_longlong: "long long", C.c_uint64: "u64",
                C.c_ulonglong: "u64", C.c_void_p: "pointer", C.c_char_p: "pointer"}


def prototypes():
    """{entry point: (return type, [argument declarations])} of the header; whatever stands in front of a `qs_name(` is its return type"""
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w \t*]*?)\b(qs_\w+)\s*\(([^()]*)\)\s*;", HEADER):
        assert name not in out, f"{name} is declared twice"
        args = [" ".join(a.split()) for a in args.split(",")]
        out[name] = (re.sub(r"\s*\*\s*", "*", " ".join(ret.split())), [] if args == ["void"] else args)
    return out


def c_kind(decl):
    """an argument's declaration -> (kind, pointee or None; "*" for a pointer to a pointer); None for a type this comparer does not know"""
    if "*" in decl:
        return "pointer", "*" if decl.count("*") > 1 else re.sub(r"\b(const|struct)\b", "", decl.split("*")[0]).strip()
    return C_KINDS.get(decl.rsplit(" ", 1)[0]), None


def mirror_kind(t):
    """a ctypes field type -> (kind, array dimensions), the terms of header_structs()"""
    dims = ()
    while issubclass(t, C.Array):
        dims, t = dims + (t._length_,), t._type_
    return "pointer" if issubclass(t, C._Pointer) else CTYPES_KINDS.get(t), dims


def signature_errors(signatures, structs, protos):
    """[(entry point, what is wrong)]: the comparer of the table with the header's prototypes"""
    names = [row[0] for row in signatures]
    errors = [(n, f"is declared in the header and has {names.count(n)} rows") for n in sorted(protos) if names.count(n) != 1]
    c_name = {mirror: cname for cname, mirror in structs.items()}
    for name, restype, argtypes in signatures:
        if name not in protos:
            errors.append((name, "has a row and no prototype in the header"))
            continue
        ret, args = protos[name]
        if RETURNS.get(ret, "a type this comparer does not know") is not restype:
            errors.append((name, f"returns {ret} in the header, the row says {restype}"))
        if len(args) != len(argtypes):
            errors.append((name, f"takes {len(args)} arguments in the header, the row has {len(argtypes)}"))
            continue
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            (kind, pointee), have = c_kind(decl), mirror_kind(t)[0]
            if kind is None or have is None:
                errors.append((name, f"argument {i}: {decl!r} / {t} is not a type this comparer knows"))
            elif kind != have:
                errors.append((name, f"argument {i} is {decl!r} in the header, the row says {t}"))
            elif have == "pointer" and getattr(t, "_type_", None) in c_name and c_name[t._type_] != pointee:
                errors.append((name, f"argument {i} points at {pointee} in the header, the row at {c_name[t._type_]}"))
            elif have == "pointer" and getattr(t, "_type_", None) in CTYPES_KINDS and CTYPES_KINDS[t._type_] != ("pointer" if pointee == "*" else C_KINDS.get(pointee)):
                errors.append((name, f"argument {i} is {decl!r} in the header, the row points at {t._type_}"))
    return errors


def test_every_prototype_agrees_with_its_row():
    protos = prototypes()
    assert len(protos) >= 90, "the header's prototypes were not parsed"
    assert signature_errors(lib.SIGNATURES, lib.STRUCTS, protos) == []
    assert lib.EXPORTS == tuple(row[0] for row in lib.SIGNATURES)


# ---- structs
def header_structs():
    """{C name: [(field, kind, array dimensions)] in order} of every struct the header gives a body; kind is None for a type nobody listed"""
    number = lambda x: int(dict(re.findall(r"^#define\s+(\w+)\s+(\d+)\s*$", HEADER, re.M)).get(x, x))
    out = {}
    for cname, body in re.findall(r"struct\s+(qs_\w+)\s*\{(.*?)\}", HEADER, flags=re.S):
        out[cname] = []
        for decl in (d for d in body.split(";") if d.strip()):
            base, first = re.fullmatch(r"\s*(.*?)([\s*]+\w+\s*(?:\[\w+\]\s*)*)", decl.split(",")[0]).groups()
            for one in [first] + decl.split(",")[1:]:
                name, dims = re.fullmatch(r"[\s*]*(\w+)\s*((?:\[\w+\]\s*)*)", one).groups()
                out[cname].append((name, "pointer" if "*" in one else C_KINDS.get(" ".join(base.split())), tuple(number(x) for x in re.findall(r"\w+", dims))))
    return out


def compiled_layouts(d, header, include, structs):
    """{C name: [sizeof, offsetof of every field, in order]} from ONE program compiled against `header`; structs: {C name: [(field, ...)]}"""
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{header}"', "int main(void) {"]
    for cname, fields in ((cname, [f[0] for f in fields]) for cname, fields in structs.items()):   # (`struct qs_x`: qs_snapshot_info alone is the entry point of that name)
        lines.append(f'printf("{cname} %zu' + " %zu" * len(fields) + f'\\n", sizeof(struct {cname})' +
                     "".join(f", offsetof(struct {cname}, {f})" for f in fields) + ");")
    (d / "layouts.c").write_text("\n".join(lines + ["return 0; }", ""]))
    subprocess.check_call(["gcc", "-I" + os.path.join(REPO, include), "-o", str(d / "layouts"), str(d / "layouts.c")])
    rows = [line.split() for line in subprocess.check_output([str(d / "layouts")]).decode().splitlines()]
    return {row[0]: [int(x) for x in row[1:]] for row in rows}


@pytest.fixture(scope="module")
def c_layouts(tmp_path_factory):
    return compiled_layouts(tmp_path_factory.mktemp("abi"), "qs_amd.h", "include", header_structs())


def layout_errors(cname, mirror, fields, numbers):
    """what is wrong with a ctypes mirror of a struct whose fields (header_structs()) and [sizeof, offsets...] the header gives"""
    names, fields, kinds = [f[0] for f in mirror._fields_], [f[0] for f in fields], [f[1:] for f in fields]
    if len(names) != len(fields):
        return [f"{cname}: the mirror has {len(names)} fields, the header {len(fields)}"]
    have = [C.sizeof(mirror)] + [getattr(mirror, f).offset if f in names else None for f in fields]
    return [f"{cname}.{f}: {n} in the header, {h} in the mirror" for f, n, h in zip(["sizeof"] + fields, numbers, have) if n != h] + \
           [f"{cname}.{f}: the mirror has {n} in its place" for f, n in zip(fields, names) if f != n] + \
           [f"{cname}.{f}: {k} in the header, {t} in the mirror" for f, k, (_, t) in zip(fields, kinds, mirror._fields_) if None in k or k != mirror_kind(t)]


def test_every_struct_of_the_header_has_a_mirror():
    assert len(header_structs()) >= 8 and set(header_structs()) == set(lib.STRUCTS)


@pytest.mark.parametrize("cname", sorted(lib.STRUCTS))
def test_struct_layout_matches_the_header(cname, c_layouts):
    assert layout_errors(cname, lib.STRUCTS[cname], header_structs()[cname], c_layouts[cname]) == []


def test_the_oracles_config_has_the_layout_of_qs_config(c_layouts, tmp_path):
    """oracle/qso.h's qso_config, field by field under qs_config's names"""
    assert compiled_layouts(tmp_path, "qso.h", "oracle", {"qso_config": header_structs()["qs_config"]})["qso_config"] == c_layouts["qs_config"]


# ---- numbers and enums
def test_abi_numbers():
    assert re.search(r"^#define QS_ABI_VERSION 9$", HEADER, re.M)
    assert lib.ABI_LIBRARY == 9 and lib.load().qs_abi_version() == 9
    assert lib.ABI_VERSION == 8   # the layouts of the Structures are that version's


def test_load_names_the_entry_a_library_lacks(monkeypatch):
    """a stand-in for ctypes.CDLL without qs_fork: refused by name under the right ABI number, by the number under another, and bound without
    it under QS_ALLOW_ABI_MISMATCH=1"""
    def stand_in(number):
        entry = type("Entry", (), {"restype": None, "argtypes": None, "__call__": lambda self: number})
        return lambda path: type("Library", (), {name: entry() for name in lib.EXPORTS if name != "qs_fork"})()
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", __file__)
    monkeypatch.delenv("QS_ALLOW_ABI_MISMATCH", raising=False)
    for number, words in ((9, "reports ABI 9 and does not export qs_fork, "), (8, "speaks ABI 8, this binding was written against ABI 9 ")):
        monkeypatch.setattr(lib, "C", types.SimpleNamespace(**{**vars(C), "CDLL": stand_in(number)}))   # lib's own name for ctypes, not ctypes
        with pytest.raises(RuntimeError, match=words + r".*build\.py --force"):
            lib.load()
    monkeypatch.setenv("QS_ALLOW_ABI_MISMATCH", "1")
    bound = lib.load()
    assert not hasattr(bound, "qs_fork") and bound.qs_step.argtypes == (C.c_void_p,) * 6 and bound.qs_destroy.restype is None


def enumerators():
    items = [x.strip() for body in re.findall(r"\benum\s*\{(.*?)\}", HEADER, flags=re.S) for x in body.split(",") if x.strip()]
    found = [re.fullmatch(r"(QS_\w+)\s*=\s*(-?\d+)", x) for x in items]
    assert all(found) and len({m.group(1) for m in found}) == len(found), "an enumerator that is not NAME = number, or one that stands twice"
    return {m.group(1): int(m.group(2)) for m in found}


ENUM_TABLES = [("QS_INFO_", vec_env.INFO), ("QS_PARAM_", vec_env.PARAM), ("QS_FRAME_", vec_env.FRAME), ("QS_COUNTER_", vec_env.QuadrupedVecEnv.COUNTERS),
               ("QS_PPO_STAT_", {name: i for i, name in enumerate(lib.PPO_STATS)}), ("QS_ARS_GET_", ars.GET), ("QS_MPC_GET_", mpc.GET),
               ("QS_POLICY_ACT_", policy.ACTIVATIONS)]


@pytest.mark.parametrize("prefix, table", ENUM_TABLES, ids=[p for p, _ in ENUM_TABLES])
def test_table_restates_the_headers_enum(prefix, table):
    want = {name[len(prefix):].lower(): value for name, value in enumerators().items() if name.startswith(prefix)}
    assert want and dict(table) == want
    assert enumerators()["QS_PPO_N_STATS"] == len(lib.PPO_STATS)


# ---- the comparers bite
def test_the_comparer_reports_planted_errors_by_name():
    vp, table = C.c_void_p, {name: (restype, args) for name, restype, args in lib.SIGNATURES}
    assert table["qs_solo_waves"][1][2] is C.c_float and table["qs_create_ex"][1][1] is C.POINTER(lib.QsRack)
    table["qs_solo_waves"] = (C.c_int, (vp, C.c_int, C.c_int))                                           # a float written as an int
    table["qs_step"] = (C.c_int, table["qs_step"][1][:-1])                                               # an argument dropped
    table["qs_create_ex"] = (C.c_int, (C.POINTER(lib.QsConfig), C.POINTER(lib.QsCamera), C.c_int, C.POINTER(vp)))   # the wrong struct
    table["qs_norm_destroy"] = (C.c_int, (vp,))                                                          # restype left at the default
    errors = signature_errors([(n, r, a) for n, (r, a) in table.items()], lib.STRUCTS, prototypes())
    assert sorted(n for n, _ in errors) == ["qs_create_ex", "qs_norm_destroy", "qs_solo_waves", "qs_step"], errors
    what = dict(errors)
    assert "argument 2 is 'float reach'" in what["qs_solo_waves"] and "6 arguments in the header, the row has 5" in what["qs_step"]
    assert "points at qs_rack in the header, the row at qs_camera" in what["qs_create_ex"] and "returns void" in what["qs_norm_destroy"]
    # a row without a prototype, a prototype without a row, a name twice, a type nobody listed
    rows = [r for r in lib.SIGNATURES if r[0] != "qs_fork"] + [("qs_nothing", C.c_int, ()), ("qs_reset", C.c_int, (vp, vp)), ("qs_get_obs", C.c_int, (vp, C.c_short))]
    names = sorted(n for n, _ in signature_errors(rows, lib.STRUCTS, prototypes()))
    assert names == ["qs_fork", "qs_get_obs", "qs_get_obs", "qs_nothing", "qs_reset"]
    rows = [(n, r, (vp, C.POINTER(C.c_int)) if n == "qs_last_step_kernel_ms" else (vp, C.c_int, vp) if n == "qs_policy_create" else a) for n, r, a in lib.SIGNATURES]
    assert dict(signature_errors(rows, lib.STRUCTS, prototypes())) == {   # an int* for a float*; nothing is said against a plain c_void_p
        "qs_last_step_kernel_ms": f"argument 1 is 'float* ms' in the header, the row points at {C.c_int}"}
    assert signature_errors([("qs_version", C.c_int, ())], lib.STRUCTS, {"qs_version": ("char*", [])}) == [("qs_version", "returns char* in the header, the row says " + str(C.c_int))]


def test_the_layout_comparer_reports_swapped_and_mistyped_fields(c_layouts):
    def errors(cname, fields):
        return layout_errors(cname, type("Planted", (C.Structure,), {"_fields_": fields}), header_structs()[cname], c_layouts[cname])
    fields, swap = dict(lib.QsPpoHyper._fields_), {"lr": "beta_two", "beta_two": "lr"}   # two doubles: the size stays, only the two offsets move
    found = errors("qs_ppo_hyper", [(swap.get(n, n), fields[swap.get(n, n)]) for n in fields])
    assert sorted(e.split(":")[0] for e in found) == ["qs_ppo_hyper.beta_two"] * 2 + ["qs_ppo_hyper.lr"] * 2, found
    # size and offsets alone let several of these through: the last member narrowed inside its padding, a float for an int, a double for a uint64
    for field, kind, wrong in (("config_digest", "u64", C.c_uint32), ("config_digest", "u64", C.c_int32), ("n_envs", "int", C.c_float), ("n_envs", "int", C.c_uint32),
                               ("layout_digest", "u64", C.c_double), ("bytes", "u64", C.c_void_p), ("bytes", "u64", C.c_int32 * 2)):
        found = errors("qs_snapshot_info", [(n, wrong if n == field else t) for n, t in lib.SnapshotInfo._fields_])
        assert f"qs_snapshot_info.{field}: ('{kind}', ()) in the header, {wrong} in the mirror" in found, found
