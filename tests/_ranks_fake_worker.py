"""Stand-in for a rank worker (tests/test_ranks_cpu.py): speaks the pipe protocol of kobato_eyes_amd/ranks.py -- 8 bytes of
length, then a pickle, on stdin / stdout -- from its own few lines, with no GPU and no library behind it.

    python _ranks_fake_worker.py --script JSON --log DIR --device D --rank K

A hashing chunk is answered from the file ids: phash = fid * 3, dhash = -fid, ok = fid % 50 != 0, in two batches with a look
for the stop message in between.  ``--script`` (JSON) says what else happens:
  "delays": {"<rank>": [seconds before answering that rank's 1st, 2nd ... hashing chunk]}
  "exit" / "sleep" / "raise": {"rank": r, "request": n, ...} -- on rank r's n-th request (from 0): leave with "status" in the
  middle of it, sleep "seconds" without a word, raise ValueError("x").
Every request is noted in DIR/rank<K>.log (one JSON line: op, workers, io_workers, stream)."""
import argparse
import json
import os
import pickle
import select
import struct
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--script", default="{}")
ap.add_argument("--log", required=True)
ap.add_argument("--device", type=int, required=True)
ap.add_argument("--rank", type=int, required=True)
args = ap.parse_args()
script = json.loads(args.script)
OUT = os.dup(1)
os.dup2(2, 1)


def read_exact(n):
    data = b""
    while len(data) < n:
        part = os.read(0, n - len(data))
        if not part:
            sys.exit(0)
        data += part
    return data


def read_message():
    (size,) = struct.unpack("<Q", read_exact(8))
    return pickle.loads(read_exact(size))


def send(message):
    body = pickle.dumps(message)
    data = struct.pack("<Q", len(body)) + body
    while data:
        data = data[os.write(OUT, data):]


def stop_waiting():
    if select.select([0], [], [], 0)[0]:
        return read_message().get("op") in ("stop", "quit")
    return False


def mine(what, count):
    rule = script.get(what)
    return rule is not None and rule["rank"] == args.rank and rule["request"] == count


def hash_chunk(request, nth):
    delays = script.get("delays", {}).get(str(args.rank), [])
    time.sleep(delays[nth] if nth < len(delays) else 0)
    first, tasks = request["first"], request["tasks"]
    fids = np.array([t[0] for t in tasks], np.int64)
    half = (len(fids) + 1) // 2
    for lo, hi in ((0, half), (half, len(fids))):
        if lo > 0 and stop_waiting():
            return {"stopped": True}
        if hi > lo:
            part = fids[lo:hi]
            send(("batch", first + lo, part, part * 3, -part, part % 50 != 0))
    return {"stopped": False}


def refine_block(request):
    pairs = request["pairs"]
    files = {p for pair in pairs for p in pair[2:4]}
    send(("run", len(pairs)))
    return {"matches": [("match", a, b, args.rank) for a, b, _, _ in pairs],
            "stats": {"pairs": len(pairs), "decodes": len(files), "gpu_decodes": 0, "fit_launches": 1, "ssim_launches": 1}}


requests = hashed = 0
while True:
    request = read_message()
    op = request.get("op")
    if op == "quit":
        break
    if op == "stop":
        continue
    with open(os.path.join(args.log, f"rank{args.rank}.log"), "a") as fh:
        fh.write(json.dumps({"op": op, "workers": request.get("workers"), "io_workers": request.get("io_workers"),
                             "stream": request.get("stream")}) + "\n")
    wanted = request.get("env", {})
    for k in [k for k in os.environ if k.startswith("KE_") and k not in wanted]:
        del os.environ[k]
    os.environ.update(wanted)
    count, requests = requests, requests + 1
    if mine("exit", count):
        os._exit(script["exit"]["status"])
    if mine("sleep", count):
        time.sleep(script["sleep"]["seconds"])
    try:
        if mine("raise", count):
            raise ValueError("x")
        if op == "hash":
            reply = hash_chunk(request, hashed)
            hashed += 1
        elif op == "refine":
            reply = refine_block(request)
        elif op == "env":
            reply = {"device": args.device, "env": {k: v for k, v in os.environ.items() if k.startswith("KE_")},
                     "other": os.environ.get("RANKS_TEST_OTHER")}
        else:
            raise KeyError(op)
        send(("done", reply))
    except Exception as exc:
        send(("error", exc))
