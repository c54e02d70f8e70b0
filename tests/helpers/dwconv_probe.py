"""Worker of tests/test_gpu_dwconv.py: the bf16 stride-1 part of the depthwise case table and the stride-2 cases (helpers/dwconv_cases.py
worker_cases) under whatever LASR_DW* switches the environment carries - the switches are read once per process, so every switch set
needs a fresh one.  Prints one JSON line: the plans this process reports, the bit-for-bit mismatches and the random pass's figures.

    dwconv_probe.py [--refs FILE] [--plan-only]

--refs: references saved by dwconv_cases.save_refs (computed here otherwise); --plan-only: the plans alone, no GPU needed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dwconv_cases as D  # noqa: E402


def main():
    args = sys.argv[1:]
    cases = D.worker_cases()
    if "--plan-only" in args:
        print(json.dumps({"plans": {c.name: D.plan_of(c) for c in cases}}))
        return
    import torch
    refs = D.load_refs(args[args.index("--refs") + 1]) if "--refs" in args else None
    res = D.run_table(cases, torch.device("cuda:0"), refs)
    torch.cuda.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
