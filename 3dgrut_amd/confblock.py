"""One checker for the trainer's config blocks.

A rule is a pair (accepts(value), words): `words` is what follows "<block>.<key> must be " in the refusal.  One definition of
"integer" (int or np.integer, never bool) and one of "number" (int, float, np.integer or np.floating, finite, never bool or str)
hold for every block; conditions between keys stay with the block that has them, after its check_block call.
"""
import math

import numpy as np


def is_integer(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)


def boolean():
    return (lambda v: isinstance(v, bool), "true or false")      # (a string such as "false" would be truthy)


def integer(ge=None, words=None):
    """An integer, >= `ge` where given."""
    return (lambda v: is_integer(v) and (ge is None or int(v) >= ge), words or ("an integer" if ge is None else f"an integer >= {ge}"))


def number(words, gt=None, ge=None, lt=None, le=None):
    """A finite number inside the interval the keywords give: gt / lt for an open end, ge / le for a closed one."""
    def accepts(v):
        return is_number(v) and (gt is None or v > gt) and (ge is None or v >= ge) and (lt is None or v < lt) and (le is None or v <= le)
    return (accepts, words)


def nullable(rule):
    return (lambda v: v is None or rule[0](v), "null or " + rule[1])


def one_of(choices):
    return (lambda v: v in choices, f"one of {choices}")


def nonempty_string():
    return (lambda v: isinstance(v, str) and bool(v), "a non-empty string")


def check_block(name, block, defaults, rules):
    """`block` against its `defaults` (no other keys) and `rules` (key -> rule); returns the block."""
    unknown = set(block) - set(defaults)
    if unknown:
        raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
    for key, (accepts, words) in rules.items():
        if not accepts(block[key]):
            raise ValueError(f"{name}.{key} must be {words}, got {block[key]!r}")
    return block
