"""The layout of the op layer (odvae_amd/ops/): one module per kernel family behind one namespace.  Host only, no library load.
  * every global name a family module reads is bound in that module (a missing import on a path no test executes);
  * everything a family module defines is re-exported by the package, as the same object;
  * the switches and the run-time state live on the package alone -- a copy in a family module would go stale under `ops.X = ...`;
  * the imports between the family modules form no cycle."""
import ast
import builtins
import dis
import importlib
import pkgutil

import pytest

# the state table of ops/__init__.py: 16 switches, 4 names of run-time state
STATE = ["UPCONV_BY_PARITY", "UPCONV_WINOGRAD4", "UPCONV_POOLED_DGRAD", "WINOGRAD", "WGRAD_WINOGRAD", "WINOGRAD4", "GN_FUSED_STATS",
         "GN_FUSED_BWD", "FUSED_SOFTMAX_BWD", "ATTN_FOLDED_SOFTMAX", "ATTN_SCORE_BUDGET", "ATTN_F32_FUSED", "LPIPS_BF16", "DISC_BF16",
         "WGRAD_1X1_GROUP", "CONV_1X1_GROUP",
         "WEIGHT_GRADIENT_ONLY", "GN_FUSED_BWD_HITS", "GN_FUSED_BWD_SUSPENDED", "_ATTN_LAST_FLAG"]


@pytest.fixture(scope="module")
def ops():
    from odvae_amd import ops
    return ops


@pytest.fixture(scope="module")
def families(ops):
    """{name: (module, source)} of every module under odvae_amd/ops/ but the package's own __init__"""
    out = {}
    for info in pkgutil.iter_modules(ops.__path__):
        mod = importlib.import_module(ops.__name__ + "." + info.name)
        with open(mod.__file__) as f:
            out[info.name] = (mod, f.read())
    assert len(out) >= 2, "no family modules found under %s" % (ops.__path__,)
    return out


def _loads(code, found):
    """(name, line) of every LOAD_GLOBAL / LOAD_NAME of this code object and the ones nested in it; a LOAD_NAME of a name the same code
    object stores (a class body reading its own attribute) is local to it"""
    own = {i.argval for i in dis.get_instructions(code) if i.opname == "STORE_NAME"} if code.co_name != "<module>" else set()
    line = code.co_firstlineno
    for ins in dis.get_instructions(code):
        line = ins.starts_line or line
        if ins.opname == "LOAD_GLOBAL" or (ins.opname == "LOAD_NAME" and ins.argval not in own):
            found.append((ins.argval, line))
    for const in code.co_consts:
        if hasattr(const, "co_code"):
            _loads(const, found)


def _defined(source):
    names = []
    for node in ast.parse(source).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.append(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            for target in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                names.extend(n.id for n in ast.walk(target) if isinstance(n, ast.Name))
    return names


def test_every_global_name_is_bound(ops, families):
    modules = dict(families, __init__=(ops, open(ops.__file__).read()))
    total, unresolved = 0, []
    for name, (mod, source) in modules.items():
        found = []
        _loads(compile(source, mod.__file__, "exec"), found)
        assert found, "%s: no global loads seen" % name
        total += len(found)
        unresolved += ["%s.py:%d %s" % (name, line, n) for n, line in found if n not in vars(mod) and not hasattr(builtins, n)]
    assert not unresolved, "names no import binds: %s" % unresolved
    assert total > 1000, "only %d loads seen in the whole op layer: the walk is not reaching the function bodies" % total


def test_the_package_re_exports_every_definition(ops, families):
    count = 0
    for name, (mod, source) in families.items():
        defined = _defined(source)
        assert defined, "%s defines nothing" % name
        for n in defined:
            assert hasattr(ops, n), "ops.%s is missing (defined in ops/%s.py)" % (n, name)
            assert getattr(ops, n) is getattr(mod, n), "ops.%s is not ops.%s.%s" % (n, name, n)
            count += 1
    assert count >= 138      # the single module this package replaced defined 158 names; 20 of them became the state table


def test_state_lives_on_the_package_alone(ops, families):
    assert len(set(STATE)) == 20
    defined_here = _defined(open(ops.__file__).read())
    for n in STATE:
        assert hasattr(ops, n), "ops.%s is gone" % n
        assert defined_here.count(n) == 1, "ops/__init__.py defines %s %d times" % (n, defined_here.count(n))
    for name, (mod, _) in families.items():
        copies = [n for n in STATE if n in vars(mod)]
        assert not copies, "ops/%s.py binds %s: a copy that `ops.X = ...` does not reach" % (name, copies)
        assert getattr(mod, "_ops", ops) is ops, "ops/%s.py: _ops is not the package" % name


def test_a_switch_set_on_the_package_reaches_the_family_module(ops, monkeypatch):
    """(reads the switch the way every family module does; no library call on this path)"""
    monkeypatch.setattr(ops, "GN_FUSED_STATS", False)
    assert not ops._gn_stats_ok(128)
    monkeypatch.setattr(ops, "GN_FUSED_STATS", True)
    assert ops._gn_stats_ok(128)
    before = ops.GN_FUSED_BWD_SUSPENDED
    with ops.gn_fused_bwd_suspended():
        assert ops.GN_FUSED_BWD_SUSPENDED == before + 1      # written in gn_link.py, seen here
    assert ops.GN_FUSED_BWD_SUSPENDED == before


def test_imports_between_family_modules_form_no_cycle(families):
    edges = {}
    for name, (_, source) in families.items():
        edges[name] = set()
        for node in ast.walk(ast.parse(source)):
            if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module:
                edges[name].add(node.module.split(".")[0])
            elif isinstance(node, ast.ImportFrom) and node.level == 1:      # `from . import x`
                edges[name].update(a.name for a in node.names)
        assert edges[name] <= set(families), "%s imports %s" % (name, edges[name] - set(families))
    done = set()
    while len(done) < len(edges):
        ready = [n for n in edges if n not in done and edges[n] <= done]
        assert ready, "import cycle among %s" % sorted(set(edges) - done)
        done.update(ready)
