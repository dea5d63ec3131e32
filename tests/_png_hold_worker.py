"""Worker of tests/test_gpu_png_deflate.py: a fresh process, because the PNG decoder reads KE_PNG_HOLD once per process.  Decodes
the valid and the random set of hand-written deflate streams in one call and writes status and a digest of the pixels per file."""
import faulthandler
import json
import os
import sys

root, out_path = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))

import test_png_cpu as T  # noqa: E402
from _png_cases import pixel_digest as digest  # noqa: E402
from kobato_eyes_amd import _native  # noqa: E402

cases = list(T.valid_cases()) + list(T.random_cases())
faulthandler.dump_traceback_later(90, exit=True)                     # the GPU step's own limit: the cases above are host work
out, status = _native.get_context(0).png_decode([c[1] for c in cases])
faulthandler.cancel_dump_traceback_later()
with open(out_path, "w") as f:
    json.dump({"hold": os.environ.get("KE_PNG_HOLD"), "status": [int(s) for s in status], "digest": [digest(a) for a in out]}, f)
