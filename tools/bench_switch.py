"""bench.py under module switches of cwfa_amd.ops that it has no flag for (bench.py itself stays as it is):

    python tools/bench_switch.py OUT_WALK -- --gpus 1 --steps 20 --warmup 3          # ops.OUT_WALK = False, then bench.py
    python tools/bench_switch.py "OUT_WALK_MT=(1, 3)" -- --steps 10 --warmup 3       # ops.OUT_WALK_MT = (1, 3)

A bare NAME turns the switch off; NAME=LITERAL assigns a Python literal.  The name must exist in cwfa_amd.ops."""
import ast
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    if "--" not in argv:
        raise SystemExit(__doc__)
    cut = argv.index("--")
    sys.path.insert(0, ROOT)
    from cwfa_amd import ops
    for item in argv[:cut]:
        name, _, lit = item.partition("=")
        if not hasattr(ops, name):
            raise SystemExit(f"cwfa_amd.ops has no switch {name!r}")
        setattr(ops, name, ast.literal_eval(lit) if lit else False)
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv[cut + 1:]
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main(sys.argv[1:])
