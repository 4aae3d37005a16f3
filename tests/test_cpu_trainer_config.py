"""The trainer's configuration surface against tests/golden/trainer_config_golden.json, which records what the trainer answered
BEFORE its config blocks moved onto confblock.check_block and its command line onto one flag table (the generator beside it says
how): every block probe, every argument vector and the parser's actions must be what they were, apart from the probes the fixture
marks (`exception`), whose new answer is asserted here too.  Then the refusals the stage table adds: the walk-based stages are
refused at configuration time where the walks do not exist, and every stage is refused on several GPUs."""
import importlib
import json
import os

import numpy as np
import pytest

from tests.test_cpu_trainer import _FakeStepper, _model, _trainer

trainer_mod = importlib.import_module("3dgrut_amd.trainer")
confblock = importlib.import_module("3dgrut_amd.confblock")

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_config_golden.json")) as f:
    GOLDEN = json.load(f)


def _nest(path, value):
    for part in reversed(path.split(".")):
        value = {part: value}
    return value


def _records():
    """The fixture's compact form (the generator's compact_blocks) as one record per probe: override, block, key, value, exception
    (the class the generator marked, or None) and what the fixture's commit answered: outcome "ok", or "error" with error_type and
    error.  An accepted probe resolved to the defaults with the override merged in (the generator asserted it; the defaults
    themselves are pinned by the argument vectors)."""
    out = []
    for block, keys in GOLDEN["blocks"].items():
        for key, entry in keys.items():
            groups = [(v, None, None) for v in entry.get("ok", [])] + [(v, None, "own") for v in entry.get("refused", [])]
            groups += [(v, "a", code) for code, values in entry.get("a", {}).items() for v in values]
            groups += [(v, m, "own" if m == "c" else None) for m in "bcd" for v in entry.get(m, [])]
            for value, marked, answer in groups:
                rec = dict(override=_nest(block, {key: value}), block=block, key=key, value=value, exception=marked, outcome="error")
                shown = "<value>" if isinstance(_decode(value), np.generic) else repr(_decode(value))
                if answer is None:
                    rec["outcome"] = "ok"
                elif answer == "own":
                    rec.update(error_type="ValueError", error=entry["own"] + ", got " + shown)
                else:
                    rec.update(error_type=GOLDEN["foreign"][answer][0], error=GOLDEN["foreign"][answer][1].format(value=_decode(value)))
                out.append(rec)
    for override, block, *answer in GOLDEN["others"]:
        rec = dict(override=override, block=block, key=None, value=None, exception=None, outcome="ok")
        if answer != ["ok"]:
            rec.update(outcome="error", error_type=answer[0], error=answer[1])
        out.append(rec)
    return out


def _expected_block(rec):
    override = _decode(rec["override"])
    method = (override.get("strategy") or {}).get("method", "GSStrategy")
    return _dig(trainer_mod._merge(trainer_mod.default_config(method), override), rec["block"])


def _decode(x):
    if isinstance(x, dict):
        if "__np__" in x:
            return np.dtype(x["__np__"]).type(x["v"])
        if "__float__" in x:
            return float(x["__float__"])
        return {k: _decode(v) for k, v in x.items()}
    return [_decode(v) for v in x] if isinstance(x, list) else x


def _dig(conf, path):
    for part in path.split("."):
        conf = (conf or {}).get(part)
    return conf


def _answer(rec):
    """(outcome, payload) of a probe now: ("ok", the resolved block) or (the exception's type name, its text)."""
    value = _decode(rec["value"])
    try:
        return "ok", _dig(trainer_mod.resolve_config(_decode(rec["override"])), rec["block"])
    except Exception as e:
        text = str(e)
        return type(e).__name__, text.replace(repr(value), "<value>") if isinstance(value, np.generic) else text


def _own_message(rec):
    """The key's own refusal of the probe's value, in the words the fixture's commit used for the values it did refuse."""
    value = _decode(rec["value"])
    return GOLDEN["blocks"][rec["block"]][rec["key"]]["own"] + ", got " + ("<value>" if isinstance(value, np.generic) else repr(value))


def _same(a, b):
    """Equality that tells 1 from True and from 1.0 and an np.int64 from an int (== does not)."""
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


RECORDS = _records()


def test_the_fixture_covers_every_key_of_the_ten_blocks():
    conf = trainer_mod.resolve_config({})
    blocks = ("pose_refinement", "exposure", "evaluation", "pose_alignment", "compaction", "selection", "features", "points", "mesh",
              "strategy.densify.error")
    for path in blocks:
        assert set(GOLDEN["blocks"][path]) == set(_dig(conf, path)) - {"bounds"}, path      # (mesh.bounds: among the other probes)
        assert any(r["block"] == path and r["outcome"] == "error" and "unknown keys" in r["error"] for r in RECORDS), path
    assert {r["exception"] for r in RECORDS} == {None, "a", "b", "c", "d"}
    assert sum(r["exception"] is not None for r in RECORDS) == 55 and len(RECORDS) == 655


@pytest.mark.parametrize("marked", [None, "a", "b", "c", "d"])
def test_block_probes(marked):
    """None: the answer is the recorded one, in outcome, exception type, text and resolved block.  a, b, d: the probe is now refused
    with a ValueError in the key's own words (a: it was a TypeError or float()'s text; b: a numeric string that was accepted;
    d: True that pose_refinement / exposure took as 1.0).  c: an np.integer strategy.densify.error refused is now accepted, and
    resolves to itself."""
    records = [r for r in RECORDS if r["exception"] == marked]
    assert records
    for rec in records:
        outcome, payload = _answer(rec)
        where = rec["override"]
        if marked is None and rec["outcome"] == "ok":
            assert outcome == "ok" and _same(payload, _expected_block(rec)), (where, outcome, payload)
        elif marked is None:
            assert (outcome, payload) == (rec["error_type"], rec["error"]), where
        elif marked == "c":
            assert rec["outcome"] == "error" and outcome == "ok" and _same(payload[rec["key"]], _decode(rec["value"])), (where, outcome, payload)
        else:
            assert (rec["outcome"] == "ok") == (marked in "bd") and (outcome, payload) == ("ValueError", _own_message(rec)), (where, outcome, payload)


def test_nothing_but_strings_and_true_became_refused():
    """Of the probes the fixture's commit accepted, the only ones refused now are numeric strings (b) and True as a number (d)."""
    for rec in RECORDS:
        if rec["outcome"] == "ok" and _answer(rec)[0] != "ok":
            value = _decode(rec["value"])
            assert rec["exception"] in ("b", "d") and (isinstance(value, str) or value is True), rec


def _flatten(conf, prefix=""):
    if not isinstance(conf, dict) or not conf:
        return {prefix[:-1]: conf}
    out = {}
    for k, v in conf.items():
        out.update(_flatten(v, f"{prefix}{k}."))
    return out


def test_argument_vectors_and_parser_actions():
    """The conf of the empty vector whole; of every other vector what the fixture says differs from it, by dotted path."""
    parser = trainer_mod.build_parser()
    conf_of = lambda argv: json.loads(json.dumps(trainer_mod.config_from_args(parser.parse_args(["--path", "scene"] + argv))))
    assert _same(conf_of([]), GOLDEN["argv_base"])
    base = _flatten(GOLDEN["argv_base"])
    assert len(GOLDEN["argv"]) == 42
    for argv, diff in GOLDEN["argv"]:
        then = {k: v for k, v in dict(base, **diff).items() if not (isinstance(v, str) and v == "<removed>")}
        assert _same(_flatten(conf_of(argv)), then), argv
    actions = []
    for action in parser._actions:
        rec = {f: getattr(action, f, None) for f in GOLDEN["parser_fields"]}
        rec["choices"] = None if rec["choices"] is None else list(rec["choices"])
        rec["type"] = None if action.type is None else action.type.__name__
        rec["action"] = type(action).__name__
        actions.append([rec[f] for f in GOLDEN["parser_fields"]])
    assert len(actions) == len(GOLDEN["parser"]) == 36
    for now, then in zip(actions, GOLDEN["parser"]):
        assert now == then, (now, then)
    assert len({flag for flag, _, _, _ in trainer_mod.FLAGS}) == len(trainer_mod.FLAGS) == len(actions) - 1      # (-h)


def test_one_definition_of_integer_and_number():
    for v in (0, -3, np.int64(7), np.int32(0)):
        assert confblock.is_integer(v) and confblock.is_number(v)
    for v in (0.5, np.float32(0.5), np.float64(-1.0)):
        assert confblock.is_number(v) and not confblock.is_integer(v)
    for v in (True, False, "1", "abc", None, float("nan"), float("inf"), np.float32("inf"), [1], 1 + 0j):
        assert not confblock.is_number(v) and not confblock.is_integer(v), v
    block = {"a": 1, "b": None}
    rules = {"a": confblock.integer(ge=1), "b": confblock.nullable(confblock.number("in (0, 1)", gt=0, lt=1))}
    assert confblock.check_block("blk", block, block, rules) is block
    with pytest.raises(ValueError, match=r"^blk: unknown keys \['c', 'd'\]$"):
        confblock.check_block("blk", {"a": 0, "d": 1, "c": 2}, block, rules)      # before any key
    with pytest.raises(ValueError, match=r"^blk\.a must be an integer >= 1, got 0$"):
        confblock.check_block("blk", {"a": 0, "b": 1}, block, rules)              # in the rules' order
    with pytest.raises(ValueError, match=r"^blk\.b must be null or in \(0, 1\), got 1$"):
        confblock.check_block("blk", {"a": 1, "b": 1}, block, rules)


STAGES = (("compaction", "compact", "compaction"), ("selection", "select_by_masks", "selection"), ("features", "fit_features", "feature fitting"),
          ("points", "export_points", "point export"), ("mesh", "export_mesh", "mesh export"))


def test_the_stage_table():
    assert tuple(s[:3] for s in trainer_mod.STAGES) == STAGES and all(s[3] is True for s in trainer_mod.STAGES)
    for _, method, _ in STAGES:
        assert callable(getattr(trainer_mod.Trainer, method))


@pytest.mark.parametrize("block,noun", [(s[0], s[2]) for s in STAGES])
def test_walk_based_stages_are_refused_at_configuration_time(block, noun):
    sorted_variant, degree3 = {"render": {"splat": {"k_buffer_size": 8}}}, {"render": {"particle_kernel_degree": 3}}
    with pytest.raises(ValueError) as e:
        trainer_mod.resolve_config(dict(sorted_variant, **{block: {"enabled": True}}))
    assert str(e.value) == f"{block}: the {noun} needs the unsorted variant (render.splat.k_buffer_size is 8)"
    with pytest.raises(ValueError) as e:
        trainer_mod.resolve_config(dict(degree3, **{block: {"enabled": True}}))
    assert str(e.value) == f"{block}: the {noun} needs render.particle_kernel_degree 2 (it is 3)"
    for scope in (sorted_variant, degree3):         # refused only when asked for
        assert trainer_mod.resolve_config(dict(scope, **{block: {"enabled": False}}))[block]["enabled"] is False
    assert trainer_mod.resolve_config({block: {"enabled": True}, "render": {"splat": {"k_buffer_size": 0}, "particle_kernel_degree": 2}})[block]["enabled"]


@pytest.mark.parametrize("block,noun", [(s[0], s[2]) for s in STAGES])
def test_stages_are_refused_on_several_gpus(block, noun):
    st = _FakeStepper(_model())
    st.world_size = 2
    with pytest.raises(ValueError) as e:
        _trainer({"n_iterations": 1, block: {"enabled": True}}, stepper=st)
    assert str(e.value) == f"{block}: data-parallel {noun} is out of scope (the stepper's world_size must be 1)"
    _trainer({"n_iterations": 1, block: {"enabled": True}})          # one GPU: accepted


def test_run_walks_the_enabled_stages_in_order_and_looks_them_up_on_the_instance():
    tr, st, _, _, _ = _trainer({"n_iterations": 2, "test_last": False, "compaction": {"enabled": True}, "features": {"enabled": True},
                                "mesh": {"enabled": True}})
    calls = []
    for _, method, _ in STAGES:
        setattr(tr, method, lambda method=method: calls.append((method, tr.global_step)))
    tr.run()
    assert calls == [("compact", 2), ("fit_features", 2), ("export_mesh", 2)] and len(st.steps) == 2
