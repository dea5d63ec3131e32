"""What the two refine seams (refine.refine_pairs, refine_parallel._thumbnails_decoded_on_gpu) do with the files a GPU decoder
hands back, held to a record of what they did before formats.seam_actions and formats.Offers existed
(tests/golden/refine_seams_golden.json, see tests/golden/README).  No GPU and no library: a stand-in context answers every
device call from the file's name and writes down what it was asked."""
import json
import os
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).parent / "golden" / "refine_seams_golden.json"
MAX_SIDE = 4096
SIDES = (MAX_SIDE, MAX_SIDE + 1, 2 * MAX_SIDE - 257, 2 * MAX_SIDE - 256)
ORIENTATIONS = (0, 1, 2, 6, 8, 9)
ORIENTED = ("jpeg",)                   # the kinds whose caveats carry the orientation in bits 8..11 (include/keyes.h)
SIDE = 32                              # the thumbnails of the luma seam
ROOT = "/nowhere/ke_refine_seams"      # no such directory: Pillow opens none of the files
SIZED = (".tif", ".tiff", ".webp")     # the files whose size is scripted, so that both seams cut more than one run
FILE_BYTES = (4 << 30) // 48 // 100    # a hundred such files fill a run of the luma seam


def _files():
    """The grid of cases, per suffix of the table: [(path, (n, status, channels, flag bits, orientation, w, h))] -- status is the
    suffix's own decoder's; the name says it all."""
    from kobato_eyes_amd.formats import FORMATS

    files, n = [], 0
    for f in FORMATS:
        if f.follows is not None:
            continue
        for suffix in f.suffixes:
            for c in (1, 3, 4):
                for st in (0, 1, 2):
                    for g in range(4):
                        for o in ORIENTATIONS if f.kind in ORIENTED else (0,):
                            for side in SIDES:
                                for w, h in ((side, 100), (100, side)):
                                    files.append((f"{ROOT}/{n:05d}_{st}{c}{g}{o}_{w}x{h}{suffix}", (n, st, c, g, o, w, h)))
                                    n += 1
    return files


def _case(path: str):
    name = os.path.basename(path).rsplit(".", 1)[0]
    n, digits, size = name.split("_")
    w, h = size.split("x")
    return (int(n),) + tuple(int(d) for d in digits) + (int(w), int(h))


def _status(n: int, st: int, kind: str) -> int:
    """A base decoder answers the status in the name; a follow-up takes, leaves or refuses by file number and kind."""
    from kobato_eyes_amd.formats import FORMATS, KINDS

    if next(f.follows for f in FORMATS if f.kind == kind) is None:
        return st
    return (n // 16 + KINDS.index(kind)) % 3


class Scripted(RuntimeError):
    pass


class StandIn:
    """Context's device calls without a device.  Every buffer is a distinct integer far from the others; ``where`` knows which
    file lies at an address and how it got there, ``offers`` every decode call, ``calls`` every other one with its batch."""

    def __init__(self, fail=None):
        self.fail = fail                                   # (kind, which of its decode calls) raises
        self.decodes = Counter()
        self.offers, self.calls = [], []
        self.handed, self.where, self.outcome, self.order = {}, {}, {}, []
        self.next = 1

    def malloc(self, nbytes=0):
        dev, self.next = self.next << 44, self.next + 1
        self.handed[dev] = 0
        return dev

    def free(self, ptr):
        self.handed[ptr] += 1                              # KeyError: never handed out

    def memcpy(self, dst, src, nbytes):
        self.calls.append(["memcpy", int(nbytes)])

    def _at(self, addr):
        rec = self.where[int(addr)]                        # KeyError: no image begins there
        assert self.handed[rec["buffer"]] == 0, "the buffer was freed before this call"
        return rec

    def decode_files_owned(self, paths, kind="jpeg", *, by_shape=False):
        from kobato_eyes_amd import _native

        assert paths and all(type(p) is str for p in paths)
        cases = [_case(p) for p in paths]
        self.decodes[kind] += 1
        raised = self.fail == (kind, self.decodes[kind])
        self.offers.append([kind, [k[0] for k in cases], raised])
        if raised:
            raise Scripted(kind)
        n, st, c, g, o, w, h = (np.array(col, np.int32) for col in zip(*cases))
        st = np.array([_status(*k[:2], kind) for k in cases], np.int32)
        nbytes = np.where(st == 0, w.astype(np.int64) * h * c, 0)
        off, _ = _native.lay_out(nbytes, (w, h, c), st != 0) if by_shape else _native.lay_out(nbytes)
        dev = self.malloc() if (st == 0).any() else 0
        for i in np.nonzero(st == 0)[0].tolist():
            self.where[dev + int(off[i])] = dict(buffer=dev, n=int(n[i]), how="decoded", w=int(w[i]), h=int(h[i]), c=int(c[i]))
        return dev, off, w, h, c, st, g | (o << 8)

    def normalise_rgb(self, src, src_offsets, widths, heights, channels, orientations, *, by_shape=False):
        from kobato_eyes_amd import _native

        self.calls.append(["normalise_rgb", len(src_offsets)])
        w, h, o = (np.asarray(a, np.int32) for a in (widths, heights, orientations))
        ow, oh = np.where(o >= 5, h, w).astype(np.int32), np.where(o >= 5, w, h).astype(np.int32)
        nbytes = ow.astype(np.int64) * oh * 3
        do, _ = _native.lay_out(nbytes, (oh, ow)) if by_shape else _native.lay_out(nbytes)
        dev = self.malloc()
        for i in range(len(do)):
            rec = self._at(src + int(src_offsets[i]))
            assert (rec["how"], rec["w"], rec["h"], rec["c"]) == ("decoded", w[i], h[i], channels[i])
            self.where[dev + int(do[i])] = dict(buffer=dev, n=rec["n"], how="normalised", w=int(ow[i]), h=int(oh[i]), c=3,
                                                o=int(o[i]), was=rec["c"])
        return dev, do, ow, oh

    def thumbnail_rgb(self, src, width, height, box, filter=0):
        self.calls.append(["thumbnail_rgb", 1])
        rec = self._at(src)
        assert (rec["w"], rec["h"], rec["c"]) == (width, height, 3)
        x, y = max(1, width * box // max(width, height)), max(1, height * box // max(width, height))
        dev = self.malloc()
        how = dict(how="shrunk") if rec["how"] == "decoded" else dict(how="turned_shrunk", o=rec["o"])
        self.where[dev] = dict(buffer=dev, n=rec["n"], w=x, h=y, c=3, **how)
        return dev, x, y

    def ssim_pairs_on_device(self, pointers, widths, heights, channels, pair_a, pair_b):
        self.calls.append(["ssim_pairs_on_device", len(pointers), len(pair_a)])
        assert channels == 3
        ns = []
        for p, w, h in zip(pointers, widths, heights):
            rec = self._at(p)
            assert (rec["w"], rec["h"], rec["c"]) == (w, h, 3)
            did = {"decoded": ["as decoded", w, h], "normalised": ["normalised", rec.get("o"), rec.get("was"), w, h],
                   "shrunk": ["shrunk", w, h], "turned_shrunk": ["turned then shrunk", rec.get("o"), w, h]}[rec["how"]]
            assert self.outcome.setdefault(rec["n"], did) == did       # a file two runs share: the same in both
            ns.append(rec["n"])
        self.order.append(ns)
        scores = np.array([(31 * ns[a] + ns[b]) % 100 / 100 for a, b in zip(pair_a, pair_b)], np.float32)
        return scores, np.array([int(ns[a] % 7 == 0) for a in pair_a], np.int32)

    def resize_luma_uniform(self, pixels, n, width, height, channels, out_w, out_h, filter=0):
        self.calls.append(["resize_luma_uniform", n])
        assert (out_w, out_h, filter) == (SIDE, SIDE, 1)
        rows = []
        for j in range(n):                                 # a run lies back to back
            rec = self._at(pixels + j * width * height * channels)
            assert (rec["w"], rec["h"], rec["c"]) == (width, height, channels)
            rows.append([rec["n"], rec.get("o", 0), width, height, rec.get("was", channels)])
        return np.array(rows, np.int64)


def _observe(monkeypatch, seam: str, fail=None, files=None) -> dict:
    """One run of a seam over the grid with the stand-in context: what it offered, what it did with every file, what it called."""
    from kobato_eyes_amd import _native, refine, refine_parallel
    from kobato_eyes_amd.formats import FORMATS

    for f in FORMATS:
        monkeypatch.delenv(f.off_switch, raising=False)
        if f.opt_in:
            monkeypatch.setenv(f.opt_in, "1")
    monkeypatch.delenv("KE_GPU_REFINE_DECODE", raising=False)

    def getsize(p):
        if not str(p).endswith(SIZED):
            raise OSError(p)
        return FILE_BYTES

    monkeypatch.setattr(os.path, "getsize", getsize)
    ctx = StandIn(fail)
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": ctx)
    files = _files() if files is None else files
    seen = {"seam": seam, "fail": list(fail) if fail else None}
    try:
        if seam == "refine":
            stats = {}
            pairs = [(a[1][0], b[1][0], a[0], b[0]) for a, b in zip(files, files[1:])]
            got = refine.refine_pairs(pairs, io_workers=2, stats=stats)
            seen["stats"] = stats
            seen["results"] = _runs([None if m is None else [m.file_id_a, m.file_id_b, None if m.ssim is None else round(m.ssim, 2),
                                                             m.is_duplicate, m.reason] for m in got])
            seen["placed_order"] = [_ranges(ns) for ns in ctx.order]
        else:
            got = refine_parallel._thumbnails_decoded_on_gpu([Path(p) for p, _ in files], SIDE, 0)
            for p, row in got.items():
                n, o, w, h, c = row.tolist()
                assert type(p) is type(Path()) and n == _case(str(p))[0]       # the thumbnail is that file's
                ctx.outcome[n] = ["turned", o, w, h] if o else ["as decoded", w, h, c]
        seen["raised"] = None
    except Scripted as exc:
        seen["raised"] = str(exc)
    seen["freed"] = sorted(set(ctx.handed.values()))       # [1]: every buffer handed out was freed, once
    seen["offers"] = [[kind, _ranges(ns), raised] for kind, ns, raised in ctx.offers]
    seen["outcomes"] = _runs([ctx.outcome.get(k[0], ["left"]) for _, k in files])
    seen["calls"] = _runs(ctx.calls)
    return json.loads(json.dumps(seen))


def _ranges(ns: list) -> list:
    """[first, last] of each stretch of consecutive numbers, in order."""
    out = []
    for n in ns:
        if out and out[-1][1] == n - 1:
            out[-1][1] = n
        else:
            out.append([n, n])
    return out


def _runs(items: list) -> dict:
    """Run-length form of a list: the distinct items, and [index into them, repeats] in order."""
    rows, seq = [], []
    for it in items:
        key = json.loads(json.dumps(it))
        if key not in rows:
            rows.append(key)
        k = rows.index(key)
        if seq and seq[-1][0] == k:
            seq[-1][1] += 1
        else:
            seq.append([k, 1])
    return {"rows": rows, "seq": seq}


def _expand(runs: dict) -> list:
    return [runs["rows"][k] for k, times in runs["seq"] for _ in range(times)]


SCENARIOS = {"refine": ("refine", None), "refine_error": ("refine", ("webpl", 2)), "refine_parallel": ("refine_parallel", ("webp", 2))}


def record() -> dict:
    """The golden file's content, from the code this is run on (tests/golden/README says on which that was)."""
    out = {}
    for name, (seam, fail) in SCENARIOS.items():
        with pytest.MonkeyPatch.context() as mp:
            out[name] = _observe(mp, seam, fail)
    return out


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_a_seam_does_with_every_file_what_it_did_before_the_table_held_the_rules(monkeypatch, golden, name):
    """Offers per decode call, the outcome and placed size of every file, every normalise / thumbnail / resize / SSIM call with
    its batch length, ``stats``, the results, and the order in which the placed files reach the SSIM call: whole-list equality
    with the record.  Beyond the record: every buffer handed out is freed exactly once -- also when the scripted decode call of
    ``refine_error`` raises, which must propagate -- and no call is handed an address whose buffer is gone (StandIn._at);
    ``refine_parallel`` skips its failed run and keeps its files from the follow-ups."""
    seam, fail = SCENARIOS[name]
    got, want = _observe(monkeypatch, seam, fail), golden[name]
    assert got["freed"] == [1]
    assert got["raised"] == ("webpl" if name == "refine_error" else None)
    for key in ("offers", "stats", "placed_order"):
        assert got.get(key) == want.get(key), key
    for key in ("outcomes", "calls", "results"):
        assert (key in got) == (key in want) and (key not in got or _expand(got[key]) == _expand(want[key])), key
    assert set(got) == set(want)
    if name == "refine_parallel":
        failed = [ns for kind, ns, raised in got["offers"] if raised]
        assert len(failed) == 1
        outcomes = _expand(got["outcomes"])                    # file n is the n-th of the grid
        assert all(outcomes[n] == ["left"] for lo, hi in failed[0] for n in range(lo, hi + 1))
        later = [r for kind, ns, _ in got["offers"] if kind in ("webpl", "webpa") for r in ns]
        assert later and not any(lo <= b and a <= hi for lo, hi in failed[0] for a, b in later)


@pytest.mark.parametrize("name", ["refine", "refine_parallel"])
def test_seam_actions_alone_gives_the_recorded_outcomes(golden, name):
    """formats.seam_actions on the arrays of each recorded decode call, no seam around it: the first decoder whose answer is not
    'leave' decides a file, and that is the outcome on record (kind of outcome, orientation, channels)."""
    from kobato_eyes_amd import formats

    seam = SCENARIOS[name][0]
    cases = {k[0]: k for _, k in _files()}
    names = {"refine": {formats.AS_DECODED: "as decoded", formats.NORMALISE: "normalised", formats.SHRINK: "shrunk",
                        formats.TURN_SHRINK: "turned then shrunk"},
             "refine_parallel": {formats.AS_DECODED: "as decoded", formats.TURN: "turned"}}[seam]
    decided = {}
    for kind, ranges, raised in golden[name]["offers"]:
        if raised:
            continue
        ks = [cases[n] for lo, hi in ranges for n in range(lo, hi + 1)]
        n, st, c, g, o, w, h = (np.array(col, np.int32) for col in zip(*ks))
        st = np.array([_status(*k[:2], kind) for k in ks], np.int32)
        action, orient = formats.seam_actions(kind, seam, w, h, c, st, g | (o << 8), MAX_SIDE)
        assert action.shape == orient.shape == n.shape
        for i in np.nonzero(action != formats.LEAVE)[0].tolist():
            if int(n[i]) in decided:
                continue
            how = names[int(action[i])]
            if how == "normalised":
                decided[int(n[i])] = [how, int(orient[i]), int(c[i])]
            elif how in ("turned", "turned then shrunk"):
                decided[int(n[i])] = [how, int(orient[i])]
            else:
                decided[int(n[i])] = [how]
    want = []
    for row in _expand(golden[name]["outcomes"]):
        want.append({"left": row[:1], "as decoded": row[:1], "shrunk": row[:1], "normalised": row[:3], "turned": row[:2],
                     "turned then shrunk": row[:2]}[row[0]])
    assert [decided.get(k[0], ["left"]) for _, k in _files()] == want


def test_every_row_of_the_table_says_what_the_seams_do_with_its_files():
    """The new columns are filled in every row, with the values the seams' literals had: the orientation number is jpeg's
    alone, the picture seam composites RGBA for png / bmp / tiff / tiffc / tiffz (unless a low flag bit is set) and webpa
    (unless the orientation bit is set) and for nobody else, the luma seam leaves webpl's transparent files alone as well as
    every kind's turned ones.  Kinds of one suffix differ only there."""
    from kobato_eyes_amd import formats as F

    rows = {f.kind: f for f in F.FORMATS}
    assert (F.CAVEAT_ORIENTATION, F.CAVEAT_TRANSPARENCY) == (1, 2)
    both = F.CAVEAT_ORIENTATION | F.CAVEAT_TRANSPARENCY
    for f in F.FORMATS:
        assert type(f.orientation_number) is bool and type(f.luma_leave) is int and f.rgba_leave in (None, F.CAVEAT_ORIENTATION, both)
    assert [k for k, f in rows.items() if f.orientation_number] == ["jpeg"]
    assert {k: f.rgba_leave for k, f in rows.items() if f.rgba_leave is not None} == \
        {"png": both, "bmp": both, "tiff": both, "tiffc": both, "tiffz": both, "webpa": F.CAVEAT_ORIENTATION}
    assert {k: f.luma_leave for k, f in rows.items() if f.luma_leave != F.CAVEAT_ORIENTATION} == {"webpl": both}
    for f in F.FORMATS:                                    # a follow-up and its base: same suffixes, and only these differ
        if f.follows:
            base = rows[f.follows]
            assert f.suffixes == base.suffixes and not f.orientation_number and not base.orientation_number
            assert (f.rgba_leave, f.luma_leave) == (base.rgba_leave, base.luma_leave) or f.kind in ("bmpx", "webpl", "webpa")
