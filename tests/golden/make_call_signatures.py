"""Writes tests/golden/call_signatures.json: for every `_MatrixExtra_*` routine of the reference's generated glue
(src/RcppExports.cpp), its arity in CallEntries[], the Rcpp type of each argument and the declared return type.

    python tests/golden/make_call_signatures.py [<reference root>]

The file holds names and type lists only.  tests/rcall.py reads it to decide which R type each recorded numpy argument
becomes when a record is replayed through the .Call shim: logical vectors are int32 in the records, as integer vectors
are, and only the signature tells them apart.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "call_signatures.json")


def _plain(t):
    t = re.sub(r"\bconst\b|&", "", t).replace("Rcpp::", "")
    return re.sub(r"\s+", "", t)


def read(glue):
    arity = {name: int(n) for name, n in re.findall(r'\{"_MatrixExtra_(\w+)",\s*\(DL_FUNC\)\s*&_MatrixExtra_\w+,\s*(\d+)\}', glue)}
    out = {}
    blocks = re.split(r"\nRcppExport SEXP _MatrixExtra_", glue)
    for prev, block in zip(blocks, blocks[1:]):
        name = block[:block.index("(")]
        body = block[:block.index("END_RCPP")]
        args = [_plain(t) for t in re.findall(r"input_parameter<\s*(.*?)\s*>::type", body)]
        proto = prev.rstrip().splitlines()[-1]                       # "Rcpp::List add_csr_elemwise(...);"
        ret = _plain(re.match(r"(.*?)\b%s\(" % re.escape(name), proto).group(1))
        assert name in arity and arity[name] == len(args), name
        out[name] = {"arity": arity[name], "args": args, "ret": ret}
    assert sorted(out) == sorted(arity)
    return out


def main(argv):
    if argv:
        reference = argv[0]
    else:
        from oracle import ref
        reference = ref.REFERENCE
    with open(os.path.join(reference, "src", "RcppExports.cpp")) as f:
        sigs = read(f.read())
    with open(OUT, "w") as f:
        f.write("{\n")                                     # one line per routine, sorted: a change shows as that line
        f.write(",\n".join("%s: %s" % (json.dumps(name), json.dumps(sigs[name], sort_keys=True)) for name in sorted(sigs)))
        f.write("\n}\n")
    print(f"{OUT}: {len(sigs)} routines")


if __name__ == "__main__":
    main(sys.argv[1:])
