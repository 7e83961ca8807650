"""Test support lives in plain modules, not in test modules: no module of tests/ that is not a test imports a test module, and the
tests of the pattern ops -- the case, GPU and ABI file of each op of FAMILY -- import none either, so editing one test module cannot
break the collection of another.  Read from the import statements of every tests/*.py, wherever in a file they stand."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILY = ("dot_attention", "dot_attention_bias", "dot_attention_dropout", "dot_attention_bf16", "dot_attention_edge", "additive_attention",
          "additive_attention_dropout", "additive_attention_bf16", "gatv2_attention", "gatv2_attention_dropout", "gatv2_attention_bf16",
          "gatv2_attention_edge", "edge_softmax", "spmm")


def _imported(path):
    """The top-level names of every module a file imports, at module level or inside a function."""
    names = set()
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            names.add(node.module.split(".")[0])
    return names


def _test_modules_imported_by(files):
    return {os.path.basename(p): sorted(n for n in _imported(p) if n.startswith("test_")) for p in files}


def test_no_support_module_imports_a_test_module():
    support = [p for p in glob.glob(os.path.join(HERE, "*.py")) if not os.path.basename(p).startswith("test_")]
    assert len(support) > 30
    assert {f: m for f, m in _test_modules_imported_by(support).items() if m} == {}


def test_no_file_of_the_pattern_family_imports_a_test_module():
    files = [os.path.join(HERE, name) for op in FAMILY for name in (f"{op}_case.py", f"test_gpu_{op}.py", f"test_{op}_abi.py")]
    assert len(files) == 42 and all(os.path.exists(p) for p in files)
    assert {f: m for f, m in _test_modules_imported_by(files).items() if m} == {}
