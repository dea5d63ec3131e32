"""Rank workers at the real-file seams: one process per entry of ``devices``, driven by one call.

``compute_signatures_mp(..., devices=[0, 1, 2])`` and ``refine_pairs(..., devices=[0, 1, 2])`` hand their work to a pool of
worker processes, each of which runs the single-device code (``fastsig._Pipeline`` / ``refine.refine_pairs``) unchanged on its own
device.  Nothing here touches a GPU: rows, scores and statuses are host data and travel over the workers' pipes.

* A worker is a fresh interpreter (``subprocess.Popen`` of ``python -m kobato_eyes_amd.ranks --device D --rank K``), never a fork
  that goes on running Python and never an exec of the caller: the caller may hold a GPU context of its own.  ``-m`` imports the
  package's Python when the worker starts; the shared library is loaded and the device opened by the first request.
* Requests and replies are length-prefixed pickles on the worker's stdin / stdout (the worker moves its own stdout out of the
  way first, so that nothing a library prints can end up in the stream).
* Every request carries the caller's ``KE_*`` environment; the worker makes its own equal to it before it runs the request (the
  seams read those variables at call time, the pool outlives calls).
* The pool is cached per ``tuple(devices)`` for the life of the process (``get_pool``), shut down by ``shutdown()`` / at exit.
  ``devices`` may name a device several times -- ``[0, 0, 0]`` is how a one-GPU box rehearses the path -- and holds at most
  ``MAX_WORKERS`` = 15 entries: with the caller that is 16 processes on the GPUs.
* No silent waits and no second tries: a worker that says nothing for ``timeout`` seconds, exits or closes its pipe while it has
  a request ends the call with ``RuntimeError`` -- every worker of the pool is terminated, the pool leaves the cache, nothing is
  dealt to another device.  A Python exception inside a worker comes back as a reply and is raised in the caller; the pool stays.
"""
from __future__ import annotations

import atexit
import bisect
import contextlib
import fcntl
import math
import os
import pickle
import select
import struct
import subprocess
import sys
import threading
import time
import traceback
from typing import Callable, List, Optional, Sequence, Tuple

MAX_WORKERS = 15                     # + the calling process = the 16 that may hold a GPU at once
DEFAULT_TIMEOUT = 600.0              # seconds a busy worker may stay silent
DEFAULT_RANK_CHUNK = 16384           # README's per-call rates are measured from this many files a call upwards
QUIT_WAIT = 2.0                      # seconds a worker gets to leave after the quit message
KILL_WAIT = 2.0                      # ... and after SIGTERM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = struct.Struct("<Q")


# ---- framing: 8 bytes of length, then a pickle
def _read_exact(fd: int, n: int, deadline: Optional[float]) -> Optional[bytes]:
    """n bytes of fd; None at end of file.  TimeoutError when ``deadline`` (time.monotonic) passes first."""
    parts = []
    while n:
        if deadline is not None:
            left = deadline - time.monotonic()
            if left <= 0 or not select.select([fd], [], [], left)[0]:
                raise TimeoutError
        part = os.read(fd, min(n, 1 << 20))
        if not part:
            return None
        parts.append(part)
        n -= len(part)
    return b"".join(parts)


def read_message(fd: int, deadline: Optional[float] = None):
    head = _read_exact(fd, _HEADER.size, deadline)
    if head is None:
        raise EOFError
    body = _read_exact(fd, _HEADER.unpack(head)[0], deadline)
    if body is None:
        raise EOFError
    return pickle.loads(body)


def write_message(fd: int, message, deadline: Optional[float] = None) -> None:
    """With a deadline ``fd`` must be non-blocking: a reader that has stopped reading raises TimeoutError, not a hang."""
    body = pickle.dumps(message, protocol=pickle.HIGHEST_PROTOCOL)
    view = memoryview(_HEADER.pack(len(body)) + body)
    while view:
        if deadline is not None:
            left = deadline - time.monotonic()
            if left <= 0 or not select.select([], [fd], [], left)[1]:
                raise TimeoutError
        try:
            view = view[os.write(fd, view):]
        except BlockingIOError:
            pass


def caller_environment() -> dict:
    return {k: v for k, v in os.environ.items() if k.startswith("KE_")}


def check_devices(devices) -> Tuple[int, ...]:
    devices = tuple(int(d) for d in devices)
    if not devices:
        raise ValueError("devices is empty: name at least one device, or pass devices=None for the single-device path")
    if len(devices) > MAX_WORKERS:
        raise ValueError(f"{len(devices)} rank workers asked for; at most {MAX_WORKERS} (with the caller: 16 processes on the GPUs)")
    return devices


# ---- the parent's side
class Worker:
    """One started worker process and the two pipe ends the parent holds."""

    def __init__(self, command: Sequence[str], device: int, rank: int) -> None:
        env = dict(os.environ)
        env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        self.device, self.rank = device, rank
        self.proc = subprocess.Popen([*command, "--device", str(device), "--rank", str(rank)], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, bufsize=0, env=env)
        self.pid = self.proc.pid
        fd = self.proc.stdin.fileno()
        fcntl.fcntl(fd, fcntl.F_SETFL, fcntl.fcntl(fd, fcntl.F_GETFL) | os.O_NONBLOCK)

    def fileno(self) -> int:
        return self.proc.stdout.fileno()

    def send(self, message, deadline: float) -> None:
        write_message(self.proc.stdin.fileno(), message, deadline)

    def recv(self, deadline: float):
        return read_message(self.proc.stdout.fileno(), deadline)

    def poll(self) -> Optional[int]:
        return self.proc.poll()

    def wait(self, seconds: float) -> Optional[int]:
        try:
            return self.proc.wait(seconds)
        except subprocess.TimeoutExpired:
            return None

    def terminate(self) -> None:
        if self.proc.poll() is None:
            self.proc.terminate()
            if self.wait(KILL_WAIT) is None:
                self.proc.kill()
                self.proc.wait()
        for pipe in (self.proc.stdin, self.proc.stdout):
            try:
                pipe.close()
            except OSError:
                pass


def worker_command() -> List[str]:
    return [sys.executable, "-m", "kobato_eyes_amd.ranks"]


_pools: dict = {}
_pools_lock = threading.Lock()


class Pool:
    """The coordinator.  ``command``: the command line of a worker (``--device D --rank K`` is appended); ``factory(device,
    rank)``: a started worker object instead (send / recv / fileno / poll / wait / terminate / pid / device / rank, as ``Worker``
    has them) -- either lets the tests put stand-ins behind it."""

    def __init__(self, devices, *, timeout: float = DEFAULT_TIMEOUT, command: Optional[Sequence[str]] = None,
                 factory: Optional[Callable[[int, int], object]] = None) -> None:
        self.devices = check_devices(devices)
        self.timeout = float(timeout)
        self.closed = False
        self._lock = threading.Lock()
        self._busy: dict = {}
        command = list(command) if command is not None else worker_command()
        make = factory or (lambda device, rank: Worker(command, device, rank))
        self.workers: list = []
        try:
            for rank, device in enumerate(self.devices):
                self.workers.append(make(device, rank))
        except BaseException:
            self.close(graceful=False)
            raise

    def close(self, graceful: bool = True) -> None:
        """Quit message, a short wait for each worker, then terminate; the pool leaves the cache."""
        with _pools_lock:
            if _pools.get(self.devices) is self:
                del _pools[self.devices]
        if self.closed:
            return
        self.closed = True
        if graceful:
            for w in self.workers:
                try:
                    w.send({"op": "quit"}, time.monotonic() + QUIT_WAIT)
                except (OSError, TimeoutError, ValueError):
                    pass
            for w in self.workers:
                w.wait(QUIT_WAIT)
        for w in self.workers:
            w.terminate()

    def _fail(self, worker, what: str):
        status = worker.poll()
        if status is None:
            status = worker.wait(0.5)                  # a pipe closes a moment before the process is gone
        self.close(graceful=False)
        state = f"exit status {status}" if status is not None else "still running, terminated"
        raise RuntimeError(f"rank worker {worker.rank} on device {worker.device} {what} ({state}); every worker of the pool "
                           f"was stopped and nothing was dealt to another device")

    def _send(self, worker, message) -> None:
        try:
            worker.send(message, time.monotonic() + self.timeout)
        except TimeoutError:
            self._fail(worker, f"did not take a message within {self.timeout:g} s")
        except (OSError, ValueError):
            self._fail(worker, "closed its pipe")

    def drive(self, next_job: Callable[[object], Optional[tuple]], on_message: Callable[[object, str, object], None],
              cancel_fn: Optional[Callable[[], bool]] = None) -> bool:
        """Deals jobs on demand and hands every message to ``on_message(tag, kind, payload)``.

        ``next_job(worker)`` -> (tag, request) or None; an idle worker is asked once at the start and after every job it
        finishes.  ``cancel_fn`` is asked after every message; once it answers true the busy workers are told to stop after
        their current batch, nothing more is dealt, and the call returns True when they have answered.  A Python exception
        inside a worker is raised here, after the other workers have been stopped the same way."""
        if self.closed:
            raise RuntimeError("this pool of rank workers has been shut down")
        with self._lock:
            try:
                return self._drive(next_job, on_message, cancel_fn)
            except BaseException:
                if not self.closed and self._busy:     # e.g. an interrupt: workers are in the middle of requests
                    self.close(graceful=False)
                raise

    def _drive(self, next_job, on_message, cancel_fn) -> bool:
        env = caller_environment()
        busy = self._busy = {}                         # worker -> [tag, when it was last heard from]
        stopping, told, error = False, False, None

        def deal(worker) -> None:
            if stopping or error is not None:
                return
            job = next_job(worker)
            if job is None:
                return
            tag, request = job
            self._send(worker, dict(request, env=env, stream=cancel_fn is not None))
            busy[worker] = [tag, time.monotonic()]

        for w in self.workers:
            deal(w)
        while busy:
            now = time.monotonic()
            for w, (_, heard) in busy.items():
                if now - heard >= self.timeout:
                    self._fail(w, f"sent nothing for {self.timeout:g} s")
            wait = min(heard + self.timeout - now for _, heard in busy.values())
            for w in select.select(list(busy), [], [], wait)[0]:
                try:
                    message = w.recv(time.monotonic() + self.timeout)
                except TimeoutError:
                    self._fail(w, f"stalled inside a message for {self.timeout:g} s")
                except (EOFError, OSError):
                    self._fail(w, "exited or closed its pipe in the middle of a request")
                except Exception as exc:
                    self._fail(w, f"sent a message that cannot be read ({type(exc).__name__}: {exc})")
                tag = busy[w][0]
                busy[w][1] = time.monotonic()
                kind = message[0]
                if kind == "error":
                    del busy[w]
                    error = error if error is not None else message[1]
                elif kind == "done":
                    del busy[w]
                    on_message(tag, "done", message[1])
                    deal(w)
                else:
                    on_message(tag, kind, message[1:])
                if cancel_fn is not None and not stopping and error is None:
                    try:
                        stopping = bool(cancel_fn())
                    except Exception as exc:           # the caller's own: raised once the workers have come to rest
                        error = exc
                if (stopping or error is not None) and not told:
                    told = True
                    for other in list(busy):
                        self._send(other, {"op": "stop"})
        if error is not None:
            raise error
        return stopping

    def ask_all(self, request: dict) -> list:
        """The same request to every worker; the replies by rank."""
        replies = [None] * len(self.workers)
        todo = {w.rank for w in self.workers}

        def next_job(worker):
            if worker.rank in todo:
                todo.discard(worker.rank)
                return worker.rank, request
            return None

        def on_message(rank, kind, payload):
            if kind == "done":
                replies[rank] = payload

        self.drive(next_job, on_message)
        return replies


def get_pool(devices, *, timeout: Optional[float] = None, command: Optional[Sequence[str]] = None,
             factory: Optional[Callable[[int, int], object]] = None) -> Pool:
    """The pool of ``tuple(devices)``, started on first use and kept for the life of the process (starting N interpreters costs
    seconds; a library scan makes many calls).  ``timeout`` given: the pool's from now on."""
    devices = check_devices(devices)
    with _pools_lock:
        pool = _pools.get(devices)
    if pool is None or pool.closed:
        pool = Pool(devices, timeout=DEFAULT_TIMEOUT if timeout is None else timeout, command=command, factory=factory)
        with _pools_lock:
            _pools[devices] = pool
    elif timeout is not None:
        pool.timeout = float(timeout)
    return pool


def cached_pool(devices) -> Optional[Pool]:
    return _pools.get(tuple(int(d) for d in devices))


@atexit.register
def shutdown() -> None:
    """Stops every pool: quit message, a short wait, then terminate."""
    for pool in list(_pools.values()):
        pool.close()
    _pools.clear()


# ---- the batch hasher over the pool
def compute_signatures(tasks, devices, *, max_workers: int, chunksize: int = 64, rank_chunk: Optional[int] = None,
                       progress: Optional[Callable[[int, int], None]] = None,
                       cancel_fn: Optional[Callable[[], bool]] = None) -> list:
    """``fastsig.compute_signatures_mp`` with ``devices``: contiguous chunks of ``rank_chunk`` tasks (default ``min(16 384,
    ceil(total / N))``) handed out on demand, each run through a worker's own ``_Pipeline`` with ``max(1, max_workers // N)``
    decoders, the rows put together by position.  With a ``cancel_fn``: the rows of the longest prefix of complete chunks."""
    from .fastsig import PROGRESS_STRIDE, _SignedRows

    devices = check_devices(devices)
    total = len(tasks)
    rows = _SignedRows()
    if total == 0 or (cancel_fn is not None and cancel_fn()):
        return rows
    pool = get_pool(devices)
    n = len(devices)
    per_rank = max(1, int(max_workers) // n)
    size = max(1, int(rank_chunk)) if rank_chunk else min(DEFAULT_RANK_CHUNK, math.ceil(total / n))
    starts = iter(range(0, total, size))
    pieces: dict = {}                                  # first position of a batch -> its (fids, phash, dhash, ok)
    complete: set = set()                              # first positions of the chunks that came back whole
    seen = {"done": 0, "mark": PROGRESS_STRIDE}

    def next_job(worker):
        first = next(starts, None)
        if first is None:
            return None
        part = [(int(fid), str(path)) for fid, path in tasks[first:first + size]]
        return first, {"op": "hash", "first": first, "tasks": part, "workers": per_rank, "chunksize": int(chunksize)}

    def report(mark: int) -> None:
        try:
            progress(mark, total)
        except Exception:
            pass

    def on_message(first, kind, payload) -> None:
        if kind == "done":
            if not payload.get("stopped"):
                complete.add(first)
            return
        if kind != "batch":
            return
        at, fids, ph, dh, ok = payload
        pieces[int(at)] = (fids, ph, dh, ok)
        seen["done"] += len(fids)
        if progress is not None:
            while seen["mark"] <= seen["done"]:
                report(seen["mark"])
                seen["mark"] += PROGRESS_STRIDE
            if seen["done"] == total and total % PROGRESS_STRIDE:
                report(total)

    pool.drive(next_job, on_message, cancel_fn)
    limit = 0
    for first in range(0, total, size):
        if first not in complete:
            break
        limit = min(total, first + size)
    import numpy as np

    for at in sorted(pieces):
        if at >= limit:
            break
        fids, ph, dh, ok = (np.asarray(a) for a in pieces[at])
        ok = ok.astype(bool)
        rows.extend(zip(fids[ok].tolist(), ph[ok].tolist(), dh[ok].tolist()))
    return rows


# ---- refine_pairs over the pool
def split_blocks(weights: Sequence[float], n: int) -> List[Tuple[int, int]]:
    """min(n, len(weights)) contiguous blocks (lo, hi) of about equal weight that cover everything once; none is empty."""
    count = len(weights)
    n = min(int(n), count)
    if n <= 0:
        return []
    if sum(weights) <= 0:
        weights = [1] * count
    cum, acc = [], 0
    for w in weights:
        acc += w
        cum.append(acc)
    cuts = [0]
    for k in range(1, n):
        target = acc * k / n                           # the cut whose weight before it comes nearest to k/n of the whole
        b = bisect.bisect_left(cum, target)
        if b == 0 or cum[b] - target < target - cum[b - 1]:
            b += 1
        cuts.append(max(cuts[-1] + 1, min(b, count - (n - k))))
    cuts.append(count)
    return list(zip(cuts[:-1], cuts[1:]))


def split_pairs(pairs: Sequence[tuple], n: int, size_of: Optional[Callable[[str], int]] = None) -> List[Tuple[int, int]]:
    """Blocks of ``pairs`` for n workers by decoded size.  A pair weighs what its files add that no earlier pair has needed
    (the blocks are contiguous because neighbouring pairs share files: a file shared across blocks is decoded in each)."""
    if size_of is None:
        from .formats import decoded_bytes_estimate as size_of
    known: set = set()
    weights = []
    for pair in pairs:
        w = 0
        for p in (str(pair[2]), str(pair[3])):
            if p not in known:
                known.add(p)
                w += size_of(p)
        weights.append(w)
    return split_blocks(weights, n)


def join_blocks(blocks: Sequence[Tuple[int, int]], replies: Sequence[dict], count: int) -> Tuple[list, dict]:
    """(matches in input order, the workers' counters summed) of the blocks' replies {"matches", "stats"}."""
    out: list = [None] * count
    stats: dict = {}
    for (lo, hi), reply in zip(blocks, replies):
        if len(reply["matches"]) != hi - lo:
            raise RuntimeError(f"a rank worker answered {len(reply['matches'])} pairs for a block of {hi - lo}")
        out[lo:hi] = reply["matches"]
        for k, v in reply["stats"].items():
            stats[k] = stats.get(k, 0) + v
    return out, stats


def refine_pairs(pairs: Sequence[tuple], devices, *, thresholds=None, io_workers: int = 8, max_decoded_bytes: int = 1 << 30,
                 stats: Optional[dict] = None, max_side: Optional[int] = None) -> list:
    """``refine.refine_pairs`` with ``devices``: one contiguous block per worker, the answers joined in input order."""
    devices = check_devices(devices)
    pairs = [(a, b, str(pa), str(pb)) for a, b, pa, pb in pairs]
    blocks = split_pairs(pairs, len(devices))
    replies: list = [None] * len(blocks)
    if blocks:
        pool = get_pool(devices)
        per_rank = max(1, int(io_workers) // len(devices))
        todo = set(range(len(blocks)))

        def next_job(worker):
            k = worker.rank
            if k not in todo:
                return None
            todo.discard(k)
            lo, hi = blocks[k]
            return k, {"op": "refine", "pairs": pairs[lo:hi], "thresholds": thresholds, "io_workers": per_rank,
                       "max_decoded_bytes": int(max_decoded_bytes), "max_side": max_side}

        def on_message(k, kind, payload) -> None:
            if kind == "done":
                replies[k] = payload

        pool.drive(next_job, on_message)
    out, summed = join_blocks(blocks, replies, len(pairs))
    if stats is not None:
        stats.update({"decodes": 0, "gpu_decodes": 0, "fit_launches": 0, "ssim_launches": 0, "pairs": 0})
        stats.update(summed)
    return out


# ---- the worker's side
def _apply_environment(wanted: dict) -> None:
    for k in [k for k in os.environ if k.startswith("KE_") and k not in wanted]:
        del os.environ[k]
    os.environ.update(wanted)


def _portable(exc: BaseException) -> BaseException:
    """The exception as it can cross the pipe, the worker's traceback in its text where the type does not survive pickling."""
    text = "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))
    try:
        pickle.loads(pickle.dumps(exc))
        return exc
    except Exception:
        return RuntimeError(f"{type(exc).__name__} in a rank worker:\n{text}")


def _op_hash(request: dict, device: int, send, stop_asked) -> dict:
    from .fastsig import _Pipeline

    tasks, first = request["tasks"], request["first"]
    pipeline = _Pipeline(tasks, request["workers"], request["chunksize"], device, stop_asked if request.get("stream") else None)
    at = first
    with contextlib.closing(pipeline.run_batches()) as batches:
        for fids, ph, dh, ok in batches:
            send(("batch", at, fids, ph, dh, ok))
            at += len(fids)
            if stop_asked():
                break
    return {"stopped": at < first + len(tasks)}


def _op_refine(request: dict, device: int, send, stop_asked) -> dict:
    from .refine import refine_pairs as on_this_device

    stats: dict = {}
    extra = {} if request.get("max_side") is None else {"max_side": request["max_side"]}
    matches = on_this_device(request["pairs"], thresholds=request["thresholds"], device=device, io_workers=request["io_workers"],
                             max_decoded_bytes=request["max_decoded_bytes"], stats=stats,
                             _after_run=lambda stop: send(("run", stop)), **extra)
    return {"matches": matches, "stats": stats}


def _op_env(request: dict, device: int, send, stop_asked) -> dict:
    return {"device": device, "pid": os.getpid(), "env": caller_environment()}


_OPS = {"hash": _op_hash, "refine": _op_refine, "env": _op_env}


def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse

    ap = argparse.ArgumentParser(prog="kobato_eyes_amd.ranks", description="a rank worker; started by the pool, not by hand")
    ap.add_argument("--device", type=int, required=True)
    ap.add_argument("--rank", type=int, default=0)
    args = ap.parse_args(argv)
    out_fd = os.dup(1)
    os.dup2(2, 1)                                      # whatever prints from here on goes to stderr, not into the stream
    state = {"stop": False, "quit": False}
    reading = threading.Lock()

    def send(message) -> None:
        write_message(out_fd, message)

    def stop_asked() -> bool:
        """Between batches: has the parent sent a stop (or gone away)?  The pipeline asks from two threads."""
        with reading:
            while not state["stop"] and select.select([0], [], [], 0)[0]:
                try:
                    op = read_message(0).get("op")
                except EOFError:
                    op = "quit"
                if op == "quit":
                    state["quit"] = True
                if op in ("stop", "quit"):
                    state["stop"] = True
        return state["stop"]

    while not state["quit"]:
        try:
            request = read_message(0)
        except EOFError:
            break
        op = request.get("op")
        if op == "quit":
            break
        if op == "stop":                               # for a request that was finished already
            continue
        try:
            _apply_environment(request.get("env", {}))
            reply = ("done", _OPS[op](request, args.device, send, stop_asked))
        except Exception as exc:
            reply = ("error", _portable(exc))
        try:
            send(reply)
        except OSError:
            break
        state["stop"] = False
    return 0


if __name__ == "__main__":
    sys.exit(main())
