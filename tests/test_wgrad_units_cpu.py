"""Row units of dense weight-gradient passes (csrc/wgrad.hip, bd_wgrad_plan), on the host with placeholder addresses.

A pass with no gathered operand runs whole rounds of 256 workgroups.  Its one-round row count R1 is the smallest multiple
of 16 (from 128 up) for which all (tile, row split) pairs are at most 256 workgroups; when R1 is long the pass takes up
to MAX_ROUNDS rounds of shorter units, as long as a unit keeps UNIT_FLOOR rows.  The rule is restated here; a pass whose
R1 is under the floor must keep the one-round plan exactly, and BD_WGRAD_ROWS keeps precedence."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROUNDS, UNIT_FLOOR = 3, 256          # kWMaxRounds, kWUnitFloor
ACTOR = [(200, 230, True), (200, 200, True), (200, 200, True), (200, 200, True), (2, 200, True)]     # (N, K, bias): six tiles


def cdiv(a, b):
    return -(-a // b)


def tiles(N, K, bias):
    """Tiles of at most 13 x 13 16-blocks; K in several tiles of at most 12 blocks (dense operands: no deep tiles here,
    which need <= 4 dpre blocks)."""
    NB, KB = cdiv(N, 16), cdiv(K + int(bias), 16)
    tk = 1 if KB <= 13 else (cdiv(KB, 36) if NB <= 4 and K % 4 == 0 else cdiv(KB, 12))
    return cdiv(NB, 13), tk


def rows_for_rounds(shapes, M, k):
    R = 128
    while sum(tn * tk for tn, tk in (tiles(*s) for s in shapes)) * cdiv(M, R) > 256 * k:
        R += 16
    return R


def rule(shapes, M):
    """(rounds, rows per workgroup) of a dense pass."""
    for k in range(MAX_ROUNDS, 1, -1):
        R = rows_for_rounds(shapes, M, k)
        if R >= UNIT_FLOOR:
            return k, R
    return 1, rows_for_rounds(shapes, M, 1)


def plan(shapes, M):
    from big_dreamer_amd import _cabi as cabi
    arr = (cabi.WgradDesc * len(shapes))()
    for d, (N, K, bias) in zip(arr, shapes):
        d.dpre, d.ldp, d.act1, d.lda1, d.M1, d.act2, d.lda2 = 0x1000, N, 0x2000, K, M, None, 0
        d.M, d.N, d.K, d.dW, d.ldw, d.db = M, N, K, 0x3000, K, (0x4000 if bias else None)
    tb, tr, wsf = C.c_int(0), C.c_int(0), C.c_size_t(0)
    assert cabi.lib.bd_wgrad_plan(arr, len(shapes), C.byref(tb), C.byref(tr), C.byref(wsf)) == 0, cabi.lib.bd_last_error()
    return [dict(rows_per=d.rows_per, splits=d.splits, tiles_n=d.tiles_n, tiles_k=d.tiles_k, block_begin=d.block_begin,
                 ws_off=d.ws_off) for d in arr], tb.value, wsf.value


def check_cover(shapes, M, ds, tb, wsf):
    off = 0
    for (N, K, bias), d in zip(shapes, ds):
        assert d["rows_per"] % 16 == 0
        assert d["splits"] * d["rows_per"] >= M > (d["splits"] - 1) * d["rows_per"]
        assert (d["tiles_n"], d["tiles_k"]) == tiles(N, K, bias)
        pitch = (K + int(bias) + 3) // 4 * 4                  # slab rows are whole float4s
        assert d["ws_off"] == off and off % 4 == 0
        off += d["splits"] * N * pitch
    assert tb == sum(d["tiles_n"] * d["tiles_k"] * d["splits"] for d in ds)
    assert wsf >= off


def test_actor_pass_takes_whole_rounds_of_shorter_units():
    M = 34300
    ds, tb, wsf = plan(ACTOR, M)
    check_cover(ACTOR, M, ds, tb, wsf)
    k, R = rule(ACTOR, M)
    assert k == MAX_ROUNDS and rows_for_rounds(ACTOR, M, 1) == 832, (k, R)
    assert all(d["rows_per"] == R for d in ds), (R, ds)
    assert 256 * (k - 1) < tb <= 256 * k, (tb, k)
    assert R >= UNIT_FLOOR


def test_passes_under_the_floor_keep_the_one_round_plan():
    # the world model's dense pass (2 450 rows) and passes around the floor: the parent's rule, restated
    wm = [(600, 200, True), (200, 1024, False), (200, 230, True), (200, 200, True), (60, 200, True), (1, 200, True)]
    for shapes, M in ((wm, 2450), (ACTOR, 2450), (ACTOR, 12000), ([(200, 200, True)], 34300), (ACTOR[:2], 34300 // 3)):
        ds, tb, wsf = plan(shapes, M)
        check_cover(shapes, M, ds, tb, wsf)
        R1 = rows_for_rounds(shapes, M, 1)
        if rule(shapes, M)[0] == 1:
            assert all(d["rows_per"] == R1 and d["splits"] == cdiv(M, R1) for d in ds), (shapes, M, R1, ds)
            assert tb <= 256 or R1 == 128
    assert rule(wm, 2450)[0] == 1 and rule(ACTOR, 12000)[0] == 1
    # the first row count at which the actor's set takes a second round, and the one before it
    M2 = next(M for M in range(16, 1 << 20, 16) if rule(ACTOR, M)[0] > 1)
    for M in (M2 - 16, M2, M2 + 5):
        ds, tb, wsf = plan(ACTOR, M)
        check_cover(ACTOR, M, ds, tb, wsf)
        assert {d["rows_per"] for d in ds} == {rule(ACTOR, M)[1]}, (M, ds)


def test_rows_override_keeps_precedence():
    code = ("import json, sys; sys.path.insert(0, %r); from tests import test_wgrad_units_cpu as T; "
            "ds, tb, wsf = T.plan(T.ACTOR, 34300); T.check_cover(T.ACTOR, 34300, ds, tb, wsf); "
            "print('PLAN ' + json.dumps([d['rows_per'] for d in ds]))" % ROOT)
    for rows, want in (("200", 208), ("1024", 1024)):
        env = {k: v for k, v in os.environ.items() if k != "BD_WGRAD_WIDE"}
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT,
                             env=dict(env, BD_WGRAD_ROWS=rows))
        assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
        got = json.loads([l for l in out.stdout.splitlines() if l.startswith("PLAN ")][-1][5:])
        assert got == [want] * len(ACTOR), (rows, got)
