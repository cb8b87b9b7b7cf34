#!/usr/bin/env python3
"""Record the layout of MiniZero's own Python network modules (network/py/create_network.py) as a data fixture:
tests/golden/ref_module_layout.json, what tests/test_pt_writer.py::test_own_writer_has_the_reference_layout compares the repo's
TorchScript writer (tests/pt_writer.py) with.  For every case of that test: the top-level class name, the state_dict as
(key, shape, dtype) in registration order, and the values of the exported getters of the scripted module.  No code is stored.

usage: python tests/golden/gen_layout_golden.py <root of the MiniZero source tree (the directory that holds minizero/)>
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_pt_writer import CASES, GETTERS  # noqa: E402


def main(ref_root):
    sys.path.insert(0, ref_root)
    from minizero.network.py.create_network import create_network
    out = {}
    for name, a in sorted(CASES.items()):
        net = create_network(*a)
        scripted = torch.jit.script(net)
        getters = GETTERS + ([] if a[12] == "alphazero" else ["get_num_action_feature_channels"])
        out[name] = {"class": type(net).__name__,
                     "state_dict": [[k, list(t.shape), str(t.dtype)] for k, t in net.state_dict().items()],
                     "getters": {g: getattr(scripted, g)() for g in getters}}
    path = os.path.join(HERE, "ref_module_layout.json")
    with open(path, "w") as f:  # one state_dict entry per line
        f.write("{\n" + ",\n".join(f" {json.dumps(name)}: {{\"class\": {json.dumps(c['class'])}, \"getters\": {json.dumps(c['getters'])},\n  \"state_dict\": [\n   " +
                                    ",\n   ".join(json.dumps(e) for e in c["state_dict"]) + "]}" for name, c in out.items()) + "\n}\n")
    print(path, len(out), "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
