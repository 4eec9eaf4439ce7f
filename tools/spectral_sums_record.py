"""The sums of BandpassEngine and PhaseLockedFilterbankEngine over seeded noise (tests/spectral_sums_cases.py), as digests.
usage: python tools/spectral_sums_record.py [--record FILE.json] [--case ID ...]

Every case is run once onto a zeroed array, public API only (spectral_sums_cases.run_case, which the test shares).  Per case the
record holds the sha256 of the result's bytes, its shape and its first 8 values as float.hex() (for diagnosis): tests/test_gpu_spectral_sums_parent.py compares digest and shape with
tests/golden/spectral_sums_parent.json for equality.  The kernels use no atomics and cut their work by the call's arguments alone, so
one commit gives one record; record the fixture from the commit whose bits are to be kept, twice, and compare the two files."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--record", metavar="FILE", help="write the records of all cases as JSON")
    ap.add_argument("--case", action="append", help="run only these cases")
    args = ap.parse_args()
    import torch

    import dspsr_amd
    import spectral_sums_cases as cases
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    out = {}
    for name in args.case or cases.IDS:
        out[name] = cases.record_of(cases.run_case(dspsr_amd, ctx, name))
        print("%-40s %s %s" % (name, out[name]["sha256"][:16], out[name]["shape"]), flush=True)
    ctx.close()
    if args.record:
        with open(args.record, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
