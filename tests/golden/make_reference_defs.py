#!/usr/bin/env python3
"""Generates tests/golden/reference_julia_defs.json: the names GaussianMarkovRandomFields.jl DEFINES under src/ and ext/
(functions, one-line methods, structs, abstract types, constants, macros) and the type parameters of its `GMRF` struct.

tests/test_julia_shim_signatures.py checks the plug-in's `G.name` uses against this index, so the suite does not need a
checkout of the reference. A name counts as defined when one of these matches it (the same rules the test applied to the
live tree):
    function|struct|mutable struct|abstract type|const|macro  [Module.]name
    [Module.]name(...) [where ...] =
    [@kwdef] [mutable] struct name
Run from the repo root with the reference checkout as argument:
    python tests/golden/make_reference_defs.py <GaussianMarkovRandomFields.jl checkout>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = r"[A-Za-z_][\w!]*"


def read_sources(ref):
    text = ""
    for base in ("src", "ext"):
        for dp, _, fs in sorted(os.walk(os.path.join(ref, base))):
            for f in sorted(fs):
                if f.endswith(".jl"):
                    text += open(os.path.join(dp, f), errors="replace").read() + "\n"
    return text


def is_defined(nm, text):
    e = re.escape(nm)
    return bool(re.search(r"(?:^|\n)\s*(?:function|struct|mutable struct|abstract type|const|macro)\s+(?:\w+\.)?%s(?![\w!])" % e, text) or
                re.search(r"(?:^|\n)\s*(?:\w+\.)?%s\([^\n]*\)\s*(?:where[^\n=]*)?=" % e, text) or
                re.search(r"(?:^|\n)\s*(?:@kwdef\s+)?(?:mutable\s+)?struct\s+%s(?![\w!])" % e, text))


def split_top(s):
    """split at commas that are not inside () {} []"""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += (ch in "({[") - (ch in ")}]")
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()] if cur.strip() else out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    text = read_sources(sys.argv[1])
    # candidates: every name in a position one of the rules can match, with and without a module prefix; each is then
    # checked with the rules themselves
    kw = r"(?:function|struct|mutable struct|abstract type|const|macro)\s+"
    cand = set()
    for pat in (kw + r"(%s)" % NAME, kw + r"\w+\.(%s)" % NAME, r"(?m)^\s*(%s)\(" % NAME, r"(?m)^\s*\w+\.(%s)\(" % NAME,
                r"struct\s+(%s)" % NAME):
        cand |= set(re.findall(pat, text))
    defined = sorted(nm for nm in cand if is_defined(nm, text))
    m = re.search(r"struct GMRF\{(.*?)\}\s*<:", text, re.S)
    params = [p.strip().split("<:")[0].strip() for p in split_top(m.group(1).replace("\n", " "))]
    out = {"what": "names defined under src/ and ext/ of GaussianMarkovRandomFields.jl (tests/golden/make_reference_defs.py)",
           "defined": defined, "gmrf_type_params": params}
    with open(os.path.join(HERE, "reference_julia_defs.json"), "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print(f"{len(defined)} names, GMRF{{{', '.join(params)}}}")


if __name__ == "__main__":
    main()
