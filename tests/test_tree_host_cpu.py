"""CPU-only checks of the arbor-tree entry points: the fourth ABI surface (include/ngtree.h against _C.TREE_SIGNATURES /
_C.TREE_NON_STATUS and the library's ngtree_ symbols, with the comparison of tests/test_host_cpu.py), every refusal that needs no GPU,
the Python wrappers' argument checks, and eval.py's new switches beside the old defaults."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from test_host_cpu import _abi_mismatches, _dynamic_symbols, built  # noqa: F401  (built: the session fixture that builds the library)

NAMES = {"ngtree_workspace_bytes", "ngtree_trace"}


def _tree_prototypes():
    """{name: (return type, [(type, parameter name), ...])} of every prototype of include/ngtree.h, as test_host_cpu._abi_prototypes
    reads ngan.h: types without `const`, the `*` attached; every `ngtree_...(` of the header has to be one of them"""
    text = open(os.path.join(ROOT, "include", "ngtree.h")).read()
    mentioned = set(re.findall(r"\b(ngtree_[a-z0-9_]+)\s*\(", text))
    code = re.sub(r"(?m)^\s*#.*$", " ", re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))

    def ctype(t):
        t = " ".join(re.sub(r"\bconst\b", " ", t).replace("*", " * ").split())
        return t.replace(" *", "*")

    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s*]+)(ngtree_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        assert name not in protos, f"{name} is declared twice"
        plist = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(.*[\s*])([A-Za-z_]\w*)\s*", p, flags=re.S)
            assert m and ctype(m.group(1)), f"{name}: cannot parse the parameter {p!r}"
            plist.append((ctype(m.group(1)), m.group(2)))
        protos[name] = (ctype(ret), plist)
    assert mentioned == set(protos), f"named with a '(' in the header but not declared: {sorted(mentioned - set(protos))}"
    return protos


def test_tree_table_follows_its_header(built):  # noqa: F811
    """ngtree.h == the TREE tables == the library's ngtree_ symbols, argument by argument; the other tables hold none of them, none of
    the other headers includes this one, the core tables keep their 185 names, and lib() binds the rows"""
    C = built._C
    protos = _tree_prototypes()
    exported = {n for n in _dynamic_symbols(C.LIB_PATH) if n.startswith("ngtree_")}
    assert _abi_mismatches(protos, C.TREE_SIGNATURES, C.TREE_NON_STATUS, exported) == []
    assert set(protos) == NAMES
    others = list(C.exported_symbols()) + list(C.EXT_SIGNATURES) + list(C.EXT_NON_STATUS) + list(C.ADA_SIGNATURES)
    assert not any(n.startswith("ngtree_") for n in others) and len(C.exported_symbols()) == 185
    for header in ("ngan.h", "nganx.h", "ngada.h"):
        assert "ngtree" not in open(os.path.join(ROOT, "include", header)).read(), header
    lib = C.lib()
    for name, row in C.TREE_SIGNATURES.items():
        assert getattr(lib, name).argtypes == row and getattr(lib, name).restype is ctypes.c_int, name
    assert lib.ngtree_workspace_bytes.argtypes == [ctypes.c_int, ctypes.c_int] and lib.ngtree_workspace_bytes.restype is ctypes.c_size_t


@pytest.mark.parametrize("table, name, perturb, word", [
    ("TREE_SIGNATURES", "ngtree_trace", lambda row: row[:8] + [ctypes.c_long] + row[9:], "`int B`"),              # B as a long
    ("TREE_SIGNATURES", "ngtree_trace", lambda row: row[:-1], "10 in the table"),                                 # the stream dropped
    ("TREE_SIGNATURES", "ngtree_trace", lambda row: row[:6] + [ctypes.c_double] + row[7:], "`double* sums`"),     # sums by value
    ("TREE_NON_STATUS", "ngtree_workspace_bytes", lambda row: (row[0], ctypes.c_int), "returns size_t"),          # the size as an int
    ("TREE_NON_STATUS", "ngtree_workspace_bytes", lambda row: (row[0] + [ctypes.c_int], row[1]), "3 in the table"),
])
def test_a_drifted_tree_row_is_reported(built, table, name, perturb, word):  # noqa: F811
    C = built._C
    protos = _tree_prototypes()
    tables = {"TREE_SIGNATURES": dict(C.TREE_SIGNATURES), "TREE_NON_STATUS": dict(C.TREE_NON_STATUS)}
    row = tables[table][name]
    tables[table][name] = perturb(list(row) if isinstance(row, list) else (list(row[0]), row[1]))
    assert tables[table][name] != row
    bad = _abi_mismatches(protos, tables["TREE_SIGNATURES"], tables["TREE_NON_STATUS"], set(protos))
    assert bad and all(line.startswith(name + ":") for line in bad) and any(word in line for line in bad), bad


def test_refusals_need_no_gpu(built):  # noqa: F811
    """null pointers, pointers off their boundary and shapes outside the domain return the documented status before anything is launched"""
    lib = built._C.lib()
    ARG, SHAPE = -1, -2                                                 # NGAN_ERR_ARG, NGAN_ERR_SHAPE (include/ngan.h)
    one = 4096                                                          # any aligned non-null address: the checks come before the launch
    names = ("skeleton", "centre", "cost", "parent", "order", "stats", "sums", "workspace")
    err = lambda: lib.ngan_last_error().decode()  # noqa: E731

    def trace(B=2, R=32, **ptr):
        return lib.ngtree_trace(*[ptr.get(n, one) for n in names], B, R, None)
    for n in names:
        if n == "order":
            continue
        assert trace(**{n: None}) == ARG and "null" in err(), n
    for n, off, word in (("skeleton", 1, "16-byte"), ("cost", 4, "16-byte"), ("parent", 8, "16-byte"), ("order", 4, "16-byte"),
                         ("workspace", 8, "16-byte"), ("sums", 4, "8-byte"), ("centre", 2, "4-byte"), ("stats", 1, "4-byte")):
        assert trace(**{n: one + off}) == ARG and word in err(), n
    for R in (8, 24, 1024, 0, -16):
        assert trace(R=R) == SHAPE and f"R={R}" in err()
        assert lib.ngtree_workspace_bytes(2, R) == 0
    for B in (0, 65536, -1):
        assert trace(B=B) == SHAPE and f"B={B}" in err()
        assert lib.ngtree_workspace_bytes(B, 32) == 0
    assert lib.ngtree_workspace_bytes(3, 64) == 17 * 3 * 64 * 64 and lib.ngtree_workspace_bytes(65535, 16) == 17 * 65535 * 256
    assert lib.ngtree_workspace_bytes(1, 512) == 17 * 512 * 512


def test_the_wrappers_refuse_wrong_arguments_before_the_library(ngan):
    M = ngan.metrics
    sk, centre = torch.zeros(2, 32, 32, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(TypeError, match="centre"):
        M.arbor_tree(sk, centre.to(torch.int64))
    with pytest.raises(TypeError, match="centre"):
        M.arbor_tree(sk, centre[:1])
    with pytest.raises(ValueError, match="R=1024"):
        M.arbor_tree(torch.zeros(1, 1024, 1024, dtype=torch.uint8), centre[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # host tensors never fall back to eager PyTorch
        M.arbor_tree(sk, centre)
    assert M.TREE_STATISTICS == ("trees", "cycles", "tips", "forks", "path_max", "path_mean", "contraction", "max_order")
    assert len(M.TREE_STATS) == 12 and M.Tree.STATISTICS is M.TREE_STATISTICS and issubclass(M.Tree, M.Skeleton)
    big = M.Tree(1024, device="cpu")
    assert not big.active and "512 x 512" in big.result()["note"] and "1024" in M.format_tree(big.result())
    from neuron_gan_amd.metric_table import METRICS
    assert len(METRICS) == 7                           # the tree is no row of the checkpoint-metric table


def test_eval_takes_the_new_switches_and_keeps_the_old_defaults(ngan):
    from neuron_gan_amd import metric_table
    p = ngan.eval.build_arg_parser()
    o = p.parse_args([])
    assert (o.tree, o.tree_seed, o.tree_min_size, o.swc, o.swc_count, o.swc_seed, o.swc_main_only) == (None, 0, 1, "", 64, 0, False)
    assert (o.n, o.output, o.weights, o.ema, o.dataset_dir, o.images) == (16, "samples_default.png", "gen_dis_default.pth", False, "", "")
    for m in metric_table.METRICS:
        assert getattr(o, m.switch) is None
        for name, _, default, _ in metric_table.settings(m)[2:]:
            assert getattr(o, name) == default
    o = p.parse_args(["--tree", "--swc", "out", "--swc_count", "5", "--swc_seed", "3", "--swc_main_only", "--tree_min_size", "4", "--tree_seed", "2"])
    assert (o.tree, o.tree_seed, o.tree_min_size, o.swc, o.swc_count, o.swc_seed, o.swc_main_only) == (8192, 2, 4, "out", 5, 3, True)
    assert p.parse_args(["--tree", "100"]).tree == 100 and p.parse_args(["--branches"]).tree is None
