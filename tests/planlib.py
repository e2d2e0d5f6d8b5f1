"""Reading the launch-plan lines the library prints on stderr (HG_DEBUG=plan: `[hg plan] ..`, HG_DEBUG=bnplan: `[hg bnplan] ..`), shared
by the kernel-level suites (test_launch_plans.py, test_transform_paths.py, test_node_reductions.py): a case runs its call through `planned`, asserts the
lines it got back, and `show_plans` prints them once the test no longer captures (pytest -rA: which launches each row ran)."""
import re

import pytest


def _val(v):
    if v.startswith("["):
        return [int(x) for x in v[1:-1].split(",") if x]
    if ".." in v:
        lo, hi = v.split("..")
        return (int(lo), int(hi))
    return int(v) if re.fullmatch(r"-?\d+", v) else v   # (a word, such as path=four, stays a word)


def plan_lines(err, token="plan"):
    """The `[hg <token>]` lines of a captured stderr as dicts: what = the line's first word ("stride", "prodsum", "ntt", "mle", ..), the
    line's fields, `ptail` for the prodsum tail."""
    out = []
    for ln in err.splitlines():
        if not ln.startswith("[hg %s] " % token):
            continue
        w = ln.split()[2:]
        d = {"what": w[0], "ptail": len(w) > 1 and w[1] == "tail", "line": ln}
        for tok in w[1:]:
            if "=" in tok:
                k, v = tok.split("=", 1)
                d[k] = _val(v)
        out.append(d)
    return out


_SEEN = []


@pytest.fixture(autouse=True)
def show_plans():
    """Prints every plan the test read, once it no longer captures (a module that imports this fixture gets it for every test)."""
    _SEEN.clear()
    yield
    print("\n".join(_SEEN))


def planned(capfd, monkeypatch, fn, label="", token="plan", describe=None):
    """Runs fn() with HG_DEBUG=<token> and returns (its result, the plan lines it printed). describe(plan): a one-line summary shown
    next to the label."""
    monkeypatch.setenv("HG_DEBUG", token)
    capfd.readouterr()
    try:
        res = fn()
    finally:
        monkeypatch.delenv("HG_DEBUG")
    plan = plan_lines(capfd.readouterr().err, token)
    _SEEN.extend(["-- %s%s" % (label, ": " + describe(plan) if describe else "")] + [l["line"] for l in plan])
    return res, plan
