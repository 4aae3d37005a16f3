"""Generate the fixture that pins the trainer's configuration surface:

    tests/golden/trainer_config_golden.json

It was written by running this file at the commit BEFORE the config blocks moved onto confblock.check_block and the command line
onto one flag table, and records what that commit answered:

  blocks   conf overrides through trainer.resolve_config: "ok" plus the resolved block, or the exception's type and text.  Every key
           of the ten checked blocks gets its default, a valid other value, True (or "false" for a boolean key), values just outside
           each bound, None, a non-numeric string, a numeric string, a float where an integer is wanted, an np.int64 and an
           np.float32; every block gets an unknown key; then the cross-key conditions and the walk-scope refusals.
  argv     argument vectors with config_from_args(build_parser().parse_args(argv)).
  parser   the parser's actions, field by field (not format_help(), whose layout depends on the terminal and the Python version).

numpy scalars are encoded by tag ({"__np__": dtype, "v": value}); where an error text quotes one, its repr (which differs between
numpy 1 and 2) is replaced by "<value>".  The file is compact (compact_blocks, compact_argv): a key's probes are grouped by their
answer, an accepted probe stands for "resolved to the defaults with the override merged in" (asserted here before it is written),
and an argument vector holds what its conf changes in the empty vector's.

`exception` marks the probes whose answer is MEANT to change (tests/test_cpu_trainer_config.py holds every other probe equal):

  a   the old answer was not the key's own message (a TypeError, or float()'s conversion text): now a ValueError with the key's own
      message.
  b   a numeric string the block took through float(): now refused with the key's own message.
  c   an np.integer that strategy.densify.error refused although every other block takes one: now accepted ("integer" has one
      definition: int or np.integer, never bool).
  d   True taken as the number 1.0 by pose_refinement and exposure, which every other block refuses: now refused with the key's own
      message ("number" has one definition: never bool).

    python tests/golden/gen_trainer_config_golden.py
"""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
trainer = importlib.import_module("3dgrut_amd.trainer")

I64, F32 = np.int64(1), np.float32(0.5)
ADAM = {"beta1": ("num", 0.5, [-0.01, 1.0]), "beta2": ("num", 0.99, [-0.01, 1.0]), "eps": ("num", 1e-8, [-1e-9, float("inf")])}
RATE = ("num", 0.01, [-1e-9, float("inf"), float("nan")])
# block path -> key -> (kind, a valid value that is not the default, values just outside the bounds)
BLOCKS = {
    "pose_refinement": dict(ADAM, enabled=("bool", True, []), lr_translation=RATE, lr_rotation=RATE,
                            start_iteration=("int", 5, [-1]), end_iteration=("int", 7, [-2])),
    "exposure": dict(ADAM, enabled=("bool", True, []), lr=RATE, start_iteration=("int", 5, [-1]), end_iteration=("int", 7, [-2])),
    "evaluation": dict(colour_corrected=("bool", True, []), ridge=("num", 1e-3, [0.0, -1.0, float("inf")])),
    "pose_alignment": dict(ADAM, enabled=("bool", True, []), validation=("bool", True, []), iterations=("int", 3, [-1]),
                           lr_translation=RATE, lr_rotation=RATE),
    "compaction": dict(enabled=("bool", True, []), keep_fraction=("num", 0.25, [0.0, 1.0001, float("nan")]),
                       score=("choice", "max_weight", ["bogus"]), min_pixels=("int", 4, [-1]), finetune_iterations=("int", 9, [-1])),
    "selection": dict(enabled=("bool", True, []), mask_suffix=("str", "_thing", [""]), threshold=("num", 0.0, [-0.01, 1.01, float("nan")]),
                      min_pixels=("int", 0, [-1])),
    "features": dict(enabled=("bool", True, []), suffix=("str", "_maps", [""]), iterations=("int", 1, [0]),
                     lr=("num", 0.5, [0.0, -1.0, float("inf")])),
    "points": dict(enabled=("bool", True, []), level=("num", 0.3, [0.0, 1.0, float("nan")]), stride=("int", 4, [0]),
                   voxel=("num", 0.05, [-0.01, float("inf")])),
    "mesh": dict(enabled=("bool", True, []), level=("num", 0.3, [0.0, 1.0, float("nan")]), resolution=("int", 64, [9]),
                 voxel=("num", 0.05, [0.0, -1.0, float("inf")]), truncation_voxels=("num", 2.5, [0.0, -1.0, float("inf")]),
                 min_count=("int", 3, [0])),
    "strategy.densify.error": dict(grow_fraction=("num", 1.0, [0.0, 1.0001, float("nan")]), score=("choice", "error_mean", ["bogus"]),
                                   min_pixels=("int", 4, [-1]), views=("int", 2, [-1]), max_n_gaussians=("int", 1000, [0])),
}
SORTED, DEGREE3 = {"render": {"splat": {"k_buffer_size": 8}}}, {"render": {"particle_kernel_degree": 3}}


def encode(x):
    if isinstance(x, dict):
        return {k: encode(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if isinstance(x, np.generic):
        return {"__np__": x.dtype.name, "v": x.item()}
    if isinstance(x, float) and not np.isfinite(x):
        return {"__float__": repr(x)}
    return x


def decode(x):
    if isinstance(x, dict):
        if "__np__" in x:
            return np.dtype(x["__np__"]).type(x["v"])
        if "__float__" in x:
            return float(x["__float__"])
        return {k: decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [decode(v) for v in x]
    return x


def nest(path, value):
    for part in reversed(path.split(".")):
        value = {part: value}
    return value


def dig(conf, path):
    for part in path.split("."):
        conf = (conf or {}).get(part)
    return conf


def probe(override, path, key=None, value=None):
    """One record: the override, the block it is about, and what resolve_config answers."""
    rec = dict(override=encode(override), block=path, key=key, value=encode(value), exception=None)
    try:
        rec.update(outcome="ok", resolved=encode(dig(trainer.resolve_config(decode(rec["override"])), path)))
    except Exception as e:      # the type is part of the record
        text = str(e)
        if isinstance(value, np.generic):
            text = text.replace(repr(value), "<value>")
        rec.update(outcome="error", error_type=type(e).__name__, error=text)
    return rec


def classify(rec, kind, value):
    """The classes of the module docstring, for a probe that sets ONE key of kind `kind` to `value`."""
    own = f"{rec['block']}.{rec['key']} must "
    numeric = kind in ("int", "num")
    if rec["outcome"] == "error" and not (rec["error_type"] == "ValueError" and rec["error"].startswith(own)) \
            and not rec["error"].startswith(rec["block"].split(".")[0]):
        return "a"
    if rec["outcome"] == "ok" and numeric and isinstance(value, str):
        return "b"
    if rec["outcome"] == "error" and kind == "int" and isinstance(value, np.integer) and rec["block"] == "strategy.densify.error":
        return "c"
    if rec["outcome"] == "ok" and numeric and value is True:
        return "d"
    return None


def block_probes():
    out = [probe({}, path) for path in BLOCKS]
    for path, keys in BLOCKS.items():
        default = dig(trainer.resolve_config({}), path)
        for key, (kind, valid, outside) in keys.items():
            values = [default[key], valid, "false" if kind == "bool" else True, None, "abc", "0.5", "3", I64, F32] + list(outside)
            if kind == "int":
                values.append(2.5)
            if kind == "bool":
                values += [0, 1]
            for value in values:
                rec = probe(nest(path, {key: value}), path, key, value)
                rec["exception"] = classify(rec, kind, value)
                out.append(rec)
        out.append(probe(nest(path, {"no_such_key": 1}), path, "no_such_key", 1))
    # ---- cross-key conditions ----
    for mesh in ({"resolution": 9}, {"resolution": 10}, {"truncation_voxels": 200}, {"resolution": 6, "truncation_voxels": 2},
                 {"resolution": 5, "truncation_voxels": 2}, {"voxel": None}, {"bounds": None}, {"bounds": [[-1, -1, -1], [1, 2, 3]]},
                 {"bounds": [[-1, -1, -1], [1, 2, -1]]}, {"bounds": [[0, 0], [1, 1]]}, {"bounds": [[0, 0, 0], [1, 1, float("inf")]]},
                 {"bounds": "abc"}, {"bounds": 5}, {"bounds": [[0, 0, 0]]}):
        out.append(probe({"mesh": mesh}, "mesh"))
    for path in ("pose_refinement", "exposure"):
        for pair in ({"start_iteration": -1}, {"end_iteration": -2}, {"end_iteration": -1}, {"end_iteration": 0},
                     {"start_iteration": 9, "end_iteration": 3}):
            out.append(probe({path: pair}, path))
    out.append(probe({"strategy": {"densify": {"error": {"max_n_gaussians": None}}}}, "strategy.densify.error"))
    for strategy in ({"densify": {"criterion": "error"}}, {"densify": {"criterion": "gradient"}}, {"densify": {"criterion": "bogus"}},
                     {"densify": {"criterion": None}}, {"densify": {"criterion": "error", "split": {"n_gaussians": 3}}},
                     {"densify": {"criterion": "gradient", "split": {"n_gaussians": 3}}},
                     {"method": "MCMCStrategy"}, {"method": "MCMCStrategy", "densify": {"criterion": "error"}},
                     {"method": "MCMCStrategy", "densify": {"criterion": "gradient", "error": {"views": -1}}}):
        out.append(probe({"strategy": strategy}, "strategy.densify"))
    # ---- the walks' scope: the unsorted variant at kernel degree 2 ----
    for scope in (SORTED, DEGREE3):
        for enabled in (True, False):
            out.append(probe(dict(scope, mesh={"enabled": enabled}), "mesh"))
        for criterion in ("error", "gradient"):
            out.append(probe(dict(scope, strategy={"densify": {"criterion": criterion}}), "strategy.densify"))
    return out


# every flag of the trainer's command line with a value for it; None: the flag takes none.  OPTIONAL: value may be left out.
FLAGS = (("--out-dir", "runs/x"), ("--n-iterations", "123"), ("--strategy", "gs"), ("--strategy", "mcmc"), ("--downsample", "2"),
         ("--test-split-interval", "4"), ("--resume", "ckpt.pt"), ("--seed", "7"), ("--background", "random"), ("--background", "white"),
         ("--refine-poses", None), ("--pose-lr-translation", "0.002"), ("--pose-lr-rotation", "0.0001"), ("--exposure", None),
         ("--exposure-lr", "0.01"), ("--cc-metrics", None), ("--aligned-metrics", None), ("--align-iterations", "5"),
         ("--compact-to", "0.25"), ("--compact-score", "max_weight"), ("--compact-finetune", "11"), ("--select-by-masks", None),
         ("--select-by-masks", "_thing"), ("--select-threshold", "0.75"), ("--fit-features", None), ("--fit-features", "_maps"),
         ("--feature-iterations", "17"), ("--feature-lr", "0.5"), ("--export-points", None), ("--points-level", "0.3"),
         ("--points-stride", "4"), ("--points-voxel", "0.05"), ("--export-mesh", None), ("--mesh-resolution", "96"),
         ("--mesh-voxel", "0.02"), ("--densify-by", "error"), ("--densify-by", "gradient"), ("--densify-grow-fraction", "0.1"),
         ("--densify-views", "2"))


def argv_probes():
    vectors = [[]] + [[flag] + ([] if value is None else [value]) for flag, value in FLAGS]
    everything, seen = [], set()
    for flag, value in reversed(FLAGS):       # the last spelling of a flag that is listed twice
        if flag not in seen and not (flag == "--strategy" and value == "mcmc"):
            seen.add(flag)
            everything += [flag] + ([] if value is None else [value])
    vectors += [everything, ["--strategy", "mcmc", "--densify-views", "3"], ["--strategy", "mcmc", "--compact-to", "0.5", "--exposure"]]
    parser = trainer.build_parser()
    return [dict(argv=v, conf=trainer.config_from_args(parser.parse_args(["--path", "scene"] + v))) for v in vectors]


PARSER_FIELDS = ("option_strings", "dest", "nargs", "const", "default", "choices", "metavar", "required", "help", "type", "action")


def parser_actions():
    """One row of PARSER_FIELDS per action; the type by its name, the action by its class name."""
    out = []
    for action in trainer.build_parser()._actions:
        rec = {f: getattr(action, f, None) for f in PARSER_FIELDS}
        rec["choices"] = None if rec["choices"] is None else list(rec["choices"])
        rec["type"] = None if action.type is None else action.type.__name__
        rec["action"] = type(action).__name__
        out.append([rec[f] for f in PARSER_FIELDS])
    return out


# ---- the file's compact form (tests/test_cpu_trainer_config.py expands it again) ----
# what the commit answered where a key had no message of its own for the value: code -> (exception type, text with {value!r})
FOREIGN = {"t": ("TypeError", "float() argument must be a string or a real number, not 'NoneType'"),
           "f": ("ValueError", "could not convert string to float: {value!r}")}
REMOVED = "<removed>"


def flatten(conf, prefix=""):
    """A nested dict as {dotted path: leaf}; an empty dict is a leaf."""
    if not isinstance(conf, dict) or not conf:
        return {prefix[:-1]: conf}
    out = {}
    for k, v in conf.items():
        out.update(flatten(v, f"{prefix}{k}."))
    return out


def expected_block(rec):
    """The block an accepted probe must resolve to: the defaults of its strategy.method with the override merged in."""
    override = decode(rec["override"])
    method = (override.get("strategy") or {}).get("method", "GSStrategy")
    return encode(dig(trainer._merge(trainer.default_config(method), override), rec["block"]))


def compact_blocks(records):
    """Single-key probes grouped per key by their answer: `ok` (resolved to the defaults with the value in place), `refused` (a
    ValueError `own` + ", got <repr of the value>"), and the marked classes — a: by FOREIGN code (what the commit answered), b and d
    (the commit said ok), c (the commit refused in the key's own words).  Every other probe: [override, block, "ok"] or [override,
    block, exception type, text].  Anything that does not fit is an error here, not a silent loss."""
    blocks, others = {}, []
    for rec in records:
        if rec["outcome"] == "ok":
            assert rec["resolved"] == expected_block(rec), rec
        if rec["key"] is None or rec["key"] == "no_such_key":
            others.append([rec["override"], rec["block"]] + (["ok"] if rec["outcome"] == "ok" else [rec["error_type"], rec["error"]]))
            continue
        entry = blocks.setdefault(rec["block"], {}).setdefault(rec["key"], {})
        value = decode(rec["value"])
        shown = "<value>" if isinstance(value, np.generic) else repr(value)
        own = rec["error"][:-len(", got " + shown)] if rec["outcome"] == "error" and rec["error"].endswith(", got " + shown) else None
        if rec["exception"] == "a":
            code = [c for c, (kind, text) in FOREIGN.items() if (kind, text.format(value=value)) == (rec["error_type"], rec["error"])]
            entry.setdefault("a", {}).setdefault(code[0], []).append(rec["value"])
        elif rec["exception"] in ("b", "d"):
            entry.setdefault(rec["exception"], []).append(rec["value"])
        elif rec["outcome"] == "ok":
            entry.setdefault("ok", []).append(rec["value"])
        elif rec["error_type"] == "ValueError" and own is not None and own.startswith(f"{rec['block']}.{rec['key']} must "):
            assert entry.setdefault("own", own) == own, rec
            entry.setdefault("c" if rec["exception"] == "c" else "refused", []).append(rec["value"])
        else:       # (refused in the words of another key or of a condition between keys)
            assert rec["exception"] is None, rec
            others.append([rec["override"], rec["block"], rec["error_type"], rec["error"]])
    return blocks, others


def compact_argv(probes):
    """The conf of the empty vector whole; of every other vector what differs from it, by dotted path (REMOVED: the path is gone)."""
    base = flatten(probes[0]["conf"])
    out = []
    for p in probes[1:]:
        flat = flatten(p["conf"])
        diff = {k: v for k, v in flat.items() if k not in base or base[k] != v or type(base[k]) is not type(v)}
        diff.update({k: REMOVED for k in base if k not in flat})
        out.append([p["argv"], diff])
    return probes[0]["conf"], out


def main():
    records = block_probes()
    blocks, others = compact_blocks(records)
    base, vectors = compact_argv(argv_probes())
    path = os.path.join(HERE, "trainer_config_golden.json")
    dumps = lambda x: json.dumps(x, separators=(",", ":"))
    with open(path, "w") as f:       # one key, one probe, one vector, one action a line
        f.write('{"foreign":' + dumps(FOREIGN) + ',\n"blocks":{\n')
        f.write(",\n".join(f'{dumps(b)}:{{\n' + ",\n".join(f" {dumps(k)}:{dumps(e)}" for k, e in keys.items()) + "}" for b, keys in blocks.items()))
        f.write('},\n"others":[\n' + ",\n".join(dumps(o) for o in others) + '],\n"argv_base":' + dumps(base) + ',\n"argv":[\n')
        f.write(",\n".join(dumps(v) for v in vectors) + '],\n"parser_fields":' + dumps(PARSER_FIELDS) + ',\n"parser":[\n')
        f.write(",\n".join(dumps(a) for a in parser_actions()) + "]}\n")
    marked = [r for r in records if r["exception"]]
    print(f"{path}: {len(records)} block probes ({len(marked)} marked), {len(vectors) + 1} argument vectors, {os.path.getsize(path)} bytes")
    for r in marked:
        print(f"  {r['exception']}  {r['block']}.{r['key']} = {decode(r['value'])!r}: {r.get('error_type', 'ok')} {r.get('error', '')}")


if __name__ == "__main__":
    main()
