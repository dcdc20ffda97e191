"""Record tests/golden/abi.json: the C-ABI as the Python binding of this tree holds it.

Every entry of bunmpc_amd._lib._SIGS (ctypes type names) and every ctypes.Structure of the module (C name, Python name, size, and per
field its name, offset, size and type name), as canonical JSON.  It imports bunmpc_amd._lib and nothing else, so it needs neither the
library nor a GPU and runs on any commit -- the table is recorded on the commit BEFORE a change to the binding and compared after it
(tests/test_abi_cpu.py).  A deliberate ABI change is re-recorded with this tool and shows up as a diff of the file.

    python tools/record_abi.py [--out tests/golden/abi.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(lib):
    """the binding of module `lib` (a bunmpc_amd._lib) as text: JSON, names sorted, one line per function and per field"""
    def name(t):
        return None if t is None else t.__name__
    structs = {s.__doc__.split(":")[0]: s for s in vars(lib).values() if isinstance(s, type) and issubclass(s, ctypes.Structure)}
    out = ['{"functions": {']
    out.append(",\n".join('  %s: %s' % (json.dumps(f), json.dumps([name(lib._SIGS[f][0]), [name(a) for a in lib._SIGS[f][1]]]))
                          for f in sorted(lib._SIGS)))
    out.append(' },\n "structs": {')
    out.append(",\n".join('  %s: {"python": "%s", "size": %d, "fields": [\n%s]}' % (
        json.dumps(c), s.__name__, ctypes.sizeof(s),
        ",\n".join("    " + json.dumps([f, getattr(s, f).offset, getattr(s, f).size, name(t)]) for f, t in s._fields_))
        for c, s in sorted(structs.items())))
    out.append(' }}\n')
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from bunmpc_amd import _lib
    text = dump(_lib)
    with open(args.out, "w") as f:
        f.write(text)
    table = json.loads(text)
    print("%d functions, %d structs -> %s" % (len(table["functions"]), len(table["structs"]), args.out))


if __name__ == "__main__":
    main()
