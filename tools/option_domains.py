"""Record what mfea_set_option accepts, for a library given by MFEA_LIB.

On a fresh handle without a mesh: every name that include/mfea_debug.h quotes
is tried; the writable options are those the library lets be set back to their
own default.  For each of them and each probe value the answer is "EINVAL" or
the value mfea_get_option reads back (after a rejected value, the read-back
must be what it was).  The defaults are recorded too.  Plain ctypes, so that
a library from an older commit can be asked as well.

    MFEA_LIB=abso/libmfea_parent.so python tools/option_domains.py --commit <hash> \
        > tests/golden/option_domains.json
"""
import argparse
import ctypes as C
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1

# every bound of a range or list check in mfea_set_option, with the value below
# and above it
PROBES = sorted({
    -2, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 44, 45, 46, 62, 63, 64, 65, 99, 100, 101,
    127, 128, 129, 192, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 1408, 2047, 2048, 2049,
    4095, 4096, 4097,
    99999, 100000, 100001, 999999, 10**6, 10**6 + 1, 1750000, 10**8 - 1, 10**8, 10**8 + 1,
    2**20 - 1, 2**20, 2**20 + 1, 2**30 - 64, 2**30 - 1, 2**30, 2**30 + 1, 2**30 + 64,
    2**31 - 3, 2**31 - 2, 2**31 - 1, 2**31, 2**40})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    a = ap.parse_args()
    lib = C.CDLL(os.environ.get("MFEA_LIB", os.path.join(REPO, "mycelium-fea-project_amd", "libmfea.so")))
    lib.mfea_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.mfea_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
    h = C.c_void_p()
    if lib.mfea_create(0, C.byref(h)) != 0:
        sys.exit("mfea_create failed")

    def get(name):
        v = C.c_int64()
        rc = lib.mfea_get_option(h, name.encode(), C.byref(v))
        return v.value if rc == 0 else None

    def put(name, value):
        return lib.mfea_set_option(h, name.encode(), value)

    header = open(os.path.join(REPO, "include", "mfea_debug.h")).read()
    names = list(dict.fromkeys(re.findall(r'"([a-z0-9_]+)"', header)))
    defaults = {}
    for n in names:
        d = get(n)
        if d is not None and put(n, d) == 0:
            defaults[n] = d
    answers = {}
    for n, d in defaults.items():
        row = []
        for p in PROBES:
            rc = put(n, p)
            if rc == EINVAL:
                if get(n) != d:
                    sys.exit(f"{n}: the rejected value {p} moved the option")
                row.append("EINVAL")
            elif rc == 0:
                row.append(get(n))
            else:
                sys.exit(f"{n} = {p}: unexpected return code {rc}")
            if put(n, d) != 0 or get(n) != d:
                sys.exit(f"{n}: the default {d} did not go back in")
        answers[n] = row
    lib.mfea_destroy(h)
    json.dump({"commit": a.commit, "probes": PROBES, "defaults": defaults, "answers": answers},
              sys.stdout, separators=(",", ":"))
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
