"""List every tensor of the reference's only shipped weight file (data, not source): name, scalar type and shape of the 348 entries of
YoloSharpDemo/Assets/PreTrainedModels/Yolov5n.bin, as the reference's own reader (Utils/Lib.cs:9-54) sees them.  tests/test_v5u.py pins the
Yolov5u tensor surface (model.0 .. model.23) to this list.  Run in the dev container (needs /root/reference); the output is committed."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from yolosharp_amd import weights_bin as W

SRC = "/root/reference/YoloSharpDemo/Assets/PreTrainedModels/Yolov5n.bin"
HERE = os.path.dirname(os.path.abspath(__file__))
with open(SRC, "rb") as f:
    total = W._leb_read(f)
    f.seek(0)
    items = [[n, int(c), [int(v) for v in a.shape]] for n, c, a in W.iter_bin(f)]
    rest = f.read()
assert len(items) == total and rest == b""
with open(os.path.join(HERE, "yolov5n_tensors.json"), "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(t, separators=(",", ":")) for t in items) + "\n]\n")
print(total, "tensors")
