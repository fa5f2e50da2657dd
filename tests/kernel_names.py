"""Kernels of the build's kernel_resources.json found by NAME (no test in here).
The file's keys are Itanium-mangled (`_ZN3apg12_GLOBAL__N_121cart_mpc_solve_
kernelILi5EEEv...`); split_key walks the length-prefixed components of the
kernel's name and gives its last one with its template arguments, so that a
resource test asks for `cart_mpc_solve_kernel` and is not handed
`cart_mpc_learnt_solve_kernel` or any other name that happens to contain it."""
import functools
import json


def _source_name(key, i):
    """`<length><name>` at key[i] -> (name, index behind it)"""
    j = i
    while j < len(key) and key[j].isdigit():
        j += 1
    if j == i:
        raise ValueError(f"no length-prefixed name at {i} in {key!r}")
    n = int(key[i:j])
    if j + n > len(key):
        raise ValueError(f"name at {i} runs past the end of {key!r}")
    return key[j:j + n], j + n


def _template_args(key, i):
    """`I <arg>* E` at key[i] -> index behind the closing E.  Arguments: integer
    and bool literals (`Li5E`, `Lb1E`, `Lin3E`), builtin types (`f`, `i`, ...),
    named types (`3Foo`, `N3apg3FooE`) and nested argument lists."""
    assert key[i] == "I"
    i += 1
    while key[i] != "E":
        i = _type_or_literal(key, i)
    return i + 1


def _type_or_literal(key, i):
    c = key[i]
    if c == "L":                                   # L <type> <value> E
        return key.index("E", i) + 1
    if c == "N":                                   # N <component>+ E
        i += 1
        while key[i] != "E":
            if key[i] == "S":                      # substitution: S_, S0_, ...
                i = key.index("_", i) + 1
                continue
            if key[i] == "L":
                i += 1
            _, i = _source_name(key, i)
            if key[i] == "I":
                i = _template_args(key, i)
        return i + 1
    if c.isdigit():
        _, i = _source_name(key, i)
        return _template_args(key, i) if key[i] == "I" else i
    if c in "PKRO":                                # pointer / const / references
        return _type_or_literal(key, i + 1)
    if c in "vwbcahstijlmxynofdegz":               # builtin types
        return i + 1
    raise ValueError(f"template argument at {i} of {key!r}: not understood")


def split_key(key):
    """(base name, template-argument string) of a mangled kernel name:
    `_ZN3apg12_GLOBAL__N_121cart_mpc_solve_kernelILi5EEEv...` ->
    ("cart_mpc_solve_kernel", "ILi5E"), two arguments -> "ILb0ELb1E", no
    template -> "".  ValueError for a key that is not such a name."""
    if not key.startswith("_Z"):
        raise ValueError(f"not an Itanium-mangled name: {key!r}")
    try:
        return _split(key)
    except IndexError:
        raise ValueError(f"mangled name ends early: {key!r}") from None


def _split(key):
    i, nested = 2, False
    if key[i] == "N":
        i, nested = i + 1, True
    name = None
    while True:
        if key[i] == "L":                          # internal linkage
            i += 1
        name, i = _source_name(key, i)
        if not nested or not key[i].isdigit() and key[i] != "L":
            break
    args = ""
    if key[i] == "I":
        end = _template_args(key, i)
        args, i = key[i:end - 1], end              # (without the list's closing E)
    if nested and key[i] != "E":
        raise ValueError(f"nested name of {key!r} does not close at {i}")
    return name, args


@functools.lru_cache(maxsize=None)
def resources():
    """kernel_resources.json of the (up-to-date) build: {mangled name: entry}"""
    from apg_trajectory_tracking_amd import build
    build.build()
    with open(build.RESOURCES) as f:
        return json.load(f)


def instances(res, base):
    """{template-argument string: entry} of every kernel of `res` whose name is
    exactly `base`"""
    out = {}
    for key, entry in res.items():
        name, args = split_key(key)
        if name == base:
            assert args not in out, (base, args)
            out[args] = entry
    return out
