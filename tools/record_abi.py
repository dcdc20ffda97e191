"""Record a golden table of the C-ABI as the Python binding of this tree holds it: tests/golden/abi.json for include/bunmpc.h, and one
table per further header (--header bunmpc_turn.h --out tests/golden/abi_turn.json).

Every function of the header's table in bunmpc_amd._lib.HEADERS (ctypes type names) and every struct (C name, Python name, size, and per
field its name, offset, size and type name), as canonical JSON.  It imports bunmpc_amd._lib and nothing else, so it needs neither the
library nor a GPU and runs on any commit -- the table is recorded on the commit BEFORE a change to the binding and compared after it
(tests/test_abi_cpu.py).  A deliberate ABI change is re-recorded with this tool and shows up as a diff of the file.

A header under include/ext/ is bound by a module of its own, bunmpc_amd/_lib_<name>.py for include/ext/bunmpc_<name>.h, whose table is its
ABI: --ext bunmpc_acyclic.h --out tests/golden/abi_acyclic.json.

    python tools/record_abi.py [--header bunmpc.h | --ext bunmpc_acyclic.h] [--out tests/golden/abi.json]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(abi):
    """one header's table `abi` (an entry of bunmpc_amd._lib.HEADERS) as text: JSON, names sorted, one line per function and per field"""
    def name(t):
        return None if t is None else t.__name__
    out = ['{"functions": {']
    out.append(",\n".join('  %s: %s' % (json.dumps(f), json.dumps([name(abi.functions[f][0]), [name(a) for a in abi.functions[f][1]]]))
                          for f in sorted(abi.functions)))
    out.append(' },\n "structs": {')
    out.append(",\n".join('  %s: {"python": "%s", "size": %d, "fields": [\n%s]}' % (
        json.dumps(c), s.__name__, ctypes.sizeof(s),
        ",\n".join("    " + json.dumps([f, getattr(s, f).offset, getattr(s, f).size, name(t)]) for f, t in s._fields_))
        for c, s in sorted(abi.structs.items())))
    out.append(' }}\n')
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--header", default="bunmpc.h")
    ap.add_argument("--ext", help="a header of include/ext/ in place of --header")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.ext:
        abi = importlib.import_module("bunmpc_amd._lib_" + args.ext[len("bunmpc_"):-len(".h")]).ABI
    else:
        from bunmpc_amd import _lib
        abi = _lib.HEADERS[args.header]
    text = dump(abi)
    with open(args.out, "w") as f:
        f.write(text)
    table = json.loads(text)
    print("%d functions, %d structs -> %s" % (len(table["functions"]), len(table["structs"]), args.out))


if __name__ == "__main__":
    main()
