"""The case table of the dense seams (gat_op_dense_*): the smallest shapes at which each branch of csrc/gat_gemm_kernels.hip's host
dispatch can still go wrong, the switch settings that select the other kernels, a Python restatement of the host rules (`pick`) and
the harness that runs a case on the GPU and judges it (`run_case`).  tests/test_dense_cases_cpu.py checks the table without a GPU
(every instantiation the dispatch can name is reached; wrong kernels fail the bar; the honest model passes it);
tests/test_dense_seams.py runs it.

A case is a dict: kind, M (rows: the streamed dimension — nodes), F, HD, part, ldx (0 = F), and per kind
    project      scratch "none" | "exact" | "short" (one float below the stated size), bf16 (also run pl_bf16 = 1 and compare bit for bit)
    grad_x       hpre (with the LeakyReLU' epilogue; rows 0..3 of hpre_prev hold +0.0, -0.0 and the smallest denormals)
    grad_w       prefill (gradW holds values the launch adds into)
    unaligned    the streamed operand (X; gPR for grad_x) starts four bytes off a 16-byte boundary: the launchers must take scalar loads
Operands follow tests/test_dense_precision.py's law (dense_ref.draw): the streamed operand over 2^+-12, the other over 2^+-6; no case
has more than 3000 x 128 outputs.  A prefilled output holds normal values of 1/16 of the product's median scale: far above the bar if
the launch dropped them, small enough that the roundings of the partial sums stay inside the bar's 1e-7."""
import functools
import hashlib
import json
import zlib

import numpy as np

import dense_ref as R

BOTH, LEFT, RIGHT = 0, 1, 2
SLOPE = 0.2


def _case(kind, M, F, HD, part=BOTH, ldx=0, what="", **kw):
    c = dict(kind=kind, M=M, F=F, HD=HD, part=part, ldx=ldx, what=what, scratch="none", bf16=False, hpre=False, prefill=False, walk=False, unaligned=False)
    c.update(kw)
    c["base"] = f"{kind}:{M}x{F}x{HD}:p{part}:ldx{ldx}"
    c["id"] = c["base"] + (f":scr={c['scratch']}" if c["scratch"] != "none" else "") + (":bf16" if c["bf16"] else "") \
        + (":hpre" if c["hpre"] else "") + (":pre" if c["prefill"] else "") + (":unaligned" if c["unaligned"] else "")
    return c


def _table():
    t = []
    P = functools.partial(_case, "project")
    t += [P(300, 100, 64, what="x3<4,8,vec4>, 44-row tail", bf16=True),
          P(257, 128, 64, what="K at the LDS limit, > 64 KiB of dynamic LDS"),
          P(200, 67, 64, what="scalar loads, 3-wide k tail"),
          P(200, 67, 64, ldx=68, what="vec4 with K % 4 != 0: the padded-pitch contract"),
          P(200, 67, 64, ldx=80, what="vec4 with K % 4 != 0, 13 padding floats"),
          P(200, 64, 32, what="NT = 2"),
          P(200, 32, 16, what="NT = 1"),
          P(200, 8, 8, what="16 of 32 columns, half a k-step", bf16=True),
          P(200, 1, 8, what="K = 1"),
          P(200, 21, 21, what="generic: 42 of 64 columns, scalar"),
          P(200, 50, 100, what="two column blocks, 72-wide tail"),
          P(213, 24, 64, part=LEFT, ldx=28, what="the shard form, left", bf16=True),
          P(71, 24, 64, part=RIGHT, ldx=28, what="the shard form, j0 = HD", bf16=True),
          P(200, 200, 64, what="K > 128 without scratch: NT3 narrowed to 2"),
          P(200, 500, 64, what="NT3 = 1, four column blocks"),
          P(200, 600, 64, what="fp32 rowgemm_kernel<4,true>, five K chunks, last 88"),
          P(200, 601, 64, what="the scalar form of the above"),
          P(300, 100, 64, unaligned=True, what="X four bytes off a 16-byte boundary: scalar loads at a pitch of whole float4s")]
    for M, F, HD, ldx, what in ((300, 1433, 64, 1436, "split-K, vec4"), (300, 1433, 64, 1433, "split-K, scalar"), (200, 500, 8, 0, "split-K, 16 of 64 columns")):
        t += [P(M, F, HD, ldx=ldx, scratch="exact", bf16=True, what=what),
              P(M, F, HD, ldx=ldx, scratch="short", bf16=True, what=what + "; scratch one float short: the streaming kernel")]
    for HD, F, what in ((64, 64, "K = 128"), (8, 64, "one k-step"), (32, 16, ""), (16, 32, ""), (21, 21, "scalar"), (64, 100, "NT = 4, column tail"),
                        (128, 64, "K = 256, narrowed block"), (320, 64, "K = 640: fp32, chunked, two-phase epilogue")):
        t += [_case("grad_x", 300, F, HD, what=what), _case("grad_x", 300, F, HD, hpre=True, what=what)]
    t += [_case("grad_x", 300, 64, 64, unaligned=True, what="gPR four bytes off a 16-byte boundary: scalar loads")]
    G = functools.partial(_case, "grad_w")
    t += [G(1000, 100, 64, what="2x2 waves, 128-wide"),
          G(1000, 100, 64, prefill=True, what="the accumulate"),
          G(1000, 100, 64, unaligned=True, what="X four bytes off a 16-byte boundary: scalar loads"),
          G(1000, 64, 64, what="BN = 64"),
          G(1000, 50, 64, what="BN = 64, scalar"),
          G(1000, 100, 64, part=LEFT, what="WM = 1"),
          G(1000, 100, 64, part=RIGHT, what="WM = 1, c_base = HD"),
          G(213, 100, 64, part=LEFT, what="the shard form"),
          G(71, 100, 64, part=RIGHT, what="the shard form"),
          G(1000, 100, 32, what="M = 64"),
          G(1000, 100, 8, what="M = 16, padding rows"),
          G(1000, 50, 21, what="scalar"),
          G(1000, 100, 100, what="M = 200, 72-row tail on the 128 tile"),
          G(1000, 100, 96, what="M = 192: the M % 128 == 64 branch, three 64-row blocks"),
          G(1000, 100, 80, part=LEFT, what=""),
          G(1000, 333, 64, what="three column blocks, scalar"),
          G(300, 1433, 64, ldx=1436, what=""),
          G(1, 100, 64), G(31, 100, 64), G(129, 100, 64),
          G(6273, 100, 64, what="50 slabs: the reduction's unrolled loop"),
          G(8300, 100, 64, what="65 slabs"),
          G(3000, 100, 64, what="GAT_GRADW_KMIN=1024: three chunks, the last 952 rows", only="kmin1024")]
    for HD in (64, 21):
        t += [_case("project_res", 300, 300, HD, what="store, accumulate, accumulate"), _case("grad_wres", 300, 300, HD, prefill=True)]
    for F in (1, 3, 8):
        t += [_case("project_res", 5000, F, 64, what="the edge-feature form PE = EA We^T"), _case("grad_wres", 5000, F, 64, prefill=True)]
    t += [_case("grad_x_res", 300, 64, 160, prefill=True, what="two chunks"), _case("grad_x_res", 300, 64, 64, prefill=True)]
    # the row-streaming cases again with 1100 rows: with GAT_RESIDENT_CAP=2 a block walks several tiles (the ring crosses tile
    # boundaries with loads in flight), and every output must be bit-identical to the uncapped run's
    walk = []
    for c in t:
        if c["kind"] in ("project", "grad_x", "project_res", "grad_x_res") and c["scratch"] != "exact" and c["M"] < 1000:
            kw = {k: c[k] for k in ("part", "ldx", "scratch", "hpre", "prefill", "unaligned")}
            walk.append(_case(c["kind"], 1100, c["F"], c["HD"], what="tile walk: " + c["what"], walk=True, **kw))
    return t + walk


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

ROWGEMM = ("project", "grad_x", "project_res", "grad_x_res")
GRADW = ("grad_w", "grad_wres")


def _splitk_rows(c):
    return c["kind"] == "project" and c["scratch"] != "none"


# (environment, tag, the cases the setting can change)
SETTINGS = [
    ({}, "default", lambda c: c.get("only") is None),
    ({"GAT_GEMM_X3": "0"}, "x3=0", lambda c: c["kind"] in ROWGEMM and not c["walk"]),
    ({"GAT_GEMM_X3": "0", "GAT_GEMM_PIPE": "0"}, "x3=0,pipe=0", lambda c: c["kind"] in ROWGEMM and not c["walk"]),
    ({"GAT_GEMM_X3": "4"}, "x3=4", lambda c: c["kind"] in ROWGEMM and not c["walk"]),
    ({"GAT_GRADW_X3": "0"}, "gradw_x3=0", lambda c: c["kind"] in GRADW and c.get("only") is None),
    ({"GAT_PROJECT_SPLITK": "0"}, "splitk=0", _splitk_rows),
    ({"GAT_SPLITK_NT": "4"}, "splitk_nt=4", _splitk_rows),
    ({"GAT_X3_KMAX": "512"}, "x3_kmax=512", _splitk_rows),
    ({"GAT_GRADW_KMIN": "1024"}, "kmin=1024", lambda c: c["kind"] == "grad_w"),
    ({"GAT_GRADW_KMIN": "32"}, "kmin=32", lambda c: c["kind"] in GRADW and c.get("only") is None),
    ({"GAT_RESIDENT_CAP": "2"}, "cap=2", lambda c: (c["walk"] or c["kind"] in GRADW) and c.get("only") is None),
]
SETTING = {tag: (env, sel) for env, tag, sel in SETTINGS}


def cases_of(tag):
    return [c for c in CASES if SETTING[tag][1](c)]


# ---- the host rules of csrc/gat_gemm_kernels.hip, restated ---------------------------------------------------------------------------
def _tf(b):
    return "true" if b else "false"


def _x3_lds(K, NT):
    return 3 * ((K + 15) // 16) * 2 * (NT * 32) * 16


def pick_rowgemm(N, K, vec4, two_phase, env):
    """run_rowgemm: N output columns, K terms, 16-byte A loads, an epilogue that reads before it writes."""
    NT = 4 if N > 64 else (2 if N > 32 else 1)
    x3 = int(env.get("GAT_GEMM_X3", "-1"))
    NT3 = NT
    while NT3 > 1 and _x3_lds(K, NT3) > 100 * 1024:
        NT3 >>= 1
    if x3 != 0 and _x3_lds(K, NT3) <= 100 * 1024:
        return f"rowgemm_x3_kernel<{NT3}, {4 if x3 == 4 else 8}, {_tf(vec4)}>"
    if not two_phase and vec4 and K <= 128 and env.get("GAT_GEMM_PIPE", "1")[0] != "0" and NT <= 2:
        return f"rowgemm_pipe_kernel<{NT}>"
    return f"rowgemm_kernel<{NT}, {_tf(vec4)}>"


def wants_splitk(M, N, K, env):
    """project_wants_splitk"""
    x3 = int(env.get("GAT_GEMM_X3", "-1"))
    kmax = int(env.get("GAT_X3_KMAX", "128")) if x3 != 0 else 128
    return env.get("GAT_PROJECT_SPLITK", "1")[0] != "0" and K > kmax and ((M + 127) // 128) * ((N + 127) // 128) < 256


def project_slab_floats(M, F, HD, part, env):
    N = 2 * HD if part == BOTH else HD
    return ((F + 127) // 128) * M * N if wants_splitk(M, N, F, env) else 0


def grad_w_bm(M):
    return 128 if (M % 128 == 0 or M % 128 > 64) else 64


def grad_w_bn(M, F):
    return 64 if (grad_w_bm(M) == 128 and F <= 64) else 128


def _ldx(c):
    return c["ldx"] or c["F"]


def scratch_floats(c, env):
    """what the case hands to the projection as its scratch capacity"""
    need = project_slab_floats(c["M"], c["F"], c["HD"], c["part"], env)
    return 0 if c["scratch"] == "none" else (need if c["scratch"] == "exact" else max(need - 1, 0))


def pick(c, env):
    """The template name the seam must report for this case under this environment: the LAST row / tile kernel of the launcher."""
    kind, M, F, HD = c["kind"], c["M"], c["F"], c["HD"]
    if kind == "project":
        N = 2 * HD if c["part"] == BOTH else HD
        vec4 = _ldx(c) % 4 == 0 and not c["unaligned"]
        need = project_slab_floats(M, F, HD, c["part"], env)
        if c["scratch"] != "none" and M > 0 and need > 0 and scratch_floats(c, env) >= need:
            if env.get("GAT_GEMM_X3", "1")[0] != "0":
                return f"project_splitk_x3_kernel<{_tf(vec4)}, {4 if env.get('GAT_SPLITK_NT') == '4' else 2}>"
            return f"project_splitk_kernel<{_tf(vec4)}>"
        return pick_rowgemm(N, F, vec4, False, env)
    if kind == "grad_x":
        return pick_rowgemm(F, 2 * HD, HD % 4 == 0 and not c["unaligned"], c["hpre"], env)
    if kind == "project_res":           # K walked in chunks of 128: the first stores, the others add (a two-phase epilogue)
        last = F - ((F - 1) // 128) * 128
        return pick_rowgemm(HD, last, _ldx(c) % 4 == 0, F > 128, env)
    if kind == "grad_x_res":
        last = HD - ((HD - 1) // 128) * 128
        return pick_rowgemm(F, last, HD % 4 == 0, True, env)
    Mc = 2 * HD if (kind == "grad_w" and c["part"] == BOTH) else HD
    vec4 = _ldx(c) % 4 == 0 and HD % 4 == 0 and not c["unaligned"]
    name = "gradw_x3_kernel" if env.get("GAT_GRADW_X3", "1")[0] != "0" else "gradw_kernel"
    return f"{name}<{_tf(vec4)}, {2 if grad_w_bm(Mc) == 128 else 1}, {grad_w_bn(Mc, F)}>"


def absolute_part_applies(c, env):
    """1e-6 * max(1, sqrt(K / 100)) is the claim of the DEFAULT kernels whose longest accumulation chain is at most 128 terms, or which
    split K into such chains (split-K projection, grad_w's slabs, the residual kernels' chunks)."""
    if env:
        return False
    if c["kind"] == "project":
        return c["F"] <= 128 or pick(c, env).startswith("project_splitk")
    if c["kind"] == "grad_x":
        return 2 * c["HD"] <= 128
    return True


# ---- inputs and references (numpy; computed once per process and shared) -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(base):
    c = next(c for c in CASES if c["base"] == base)
    rng = np.random.default_rng(zlib.crc32(base.encode()))
    kind, M, F, HD = c["kind"], c["M"], c["F"], c["HD"]
    d = {}
    if kind == "project":
        d["x"] = R.draw(rng, (M, F), 12)
        d["W"] = (R.draw(rng, (HD, 2 * F), 6) * np.float32((2.0 / (F + HD)) ** 0.5)).astype(np.float32)
    elif kind == "grad_x":
        d["gpl"], d["gpr"] = R.draw(rng, (M, HD), 12), R.draw(rng, (M, HD), 12)
        d["W"] = (R.draw(rng, (HD, 2 * F), 6) * np.float32((2.0 / (F + HD)) ** 0.5)).astype(np.float32)
        h = rng.standard_normal((M, F)).astype(np.float32)
        h[0, :] = 0.0
        h[1, :] = -0.0
        h[2, :] = np.float32(1e-45)                  # the smallest denormal: > 0
        h[3, :] = np.float32(-1e-45)
        d["hpre"] = h
    elif kind in GRADW:
        d["gpl"], d["gpr"] = R.draw(rng, (M, HD), 12), R.draw(rng, (M, HD), 12)
        d["x"] = R.draw(rng, (M, F), 6)
    elif kind == "project_res":
        d["x"] = R.draw(rng, (M, F), 12)
        d["Wres"] = (R.draw(rng, (HD, F), 6) * np.float32((2.0 / (F + HD)) ** 0.5)).astype(np.float32)
    else:
        d["g"] = R.draw(rng, (M, HD), 12)
        d["Wres"] = (R.draw(rng, (HD, F), 6) * np.float32((2.0 / (F + HD)) ** 0.5)).astype(np.float32)
    return d


def operands(c):
    """{output name: (a [rows, K], b [cols, K])}: every output of the case is a b^T of these fp32 operands."""
    d = inputs(c["base"])
    kind, F, HD, part = c["kind"], c["F"], c["HD"], c["part"]
    if kind == "project":
        o = {}
        if part != RIGHT:
            o["PL"] = (d["x"], d["W"][:, :F])
        if part != LEFT:
            o["PR"] = (d["x"], d["W"][:, F:])
        return o
    if kind == "grad_x":
        return {"gprev": (np.concatenate([d["gpl"], d["gpr"]], axis=1), np.concatenate([d["W"][:, :F], d["W"][:, F:]], axis=0).T)}
    if kind == "grad_w":
        o = {}
        xt = np.ascontiguousarray(d["x"].T)
        if part != RIGHT:
            o["L"] = (np.ascontiguousarray(d["gpl"].T), xt)
        if part != LEFT:
            o["R"] = (np.ascontiguousarray(d["gpr"].T), xt)
        return o
    if kind == "grad_wres":
        return {"gradWres": (np.ascontiguousarray(d["gpl"].T), np.ascontiguousarray(d["x"].T))}
    if kind == "project_res":
        return {"R": (d["x"], d["Wres"])}
    return {"gx": (d["g"], np.ascontiguousarray(d["Wres"].T))}


@functools.lru_cache(maxsize=None)
def _reference(base, hpre, prefill):
    c = next(c for c in CASES if c["base"] == base and c["hpre"] == hpre and c["prefill"] == prefill)
    d = inputs(base)
    ref = {}
    for name, (a, b) in operands(c).items():
        exact, scale = R.product(a, b)
        K = a.shape[1]
        rc = R._chain_ratio(a, b, exact, scale) if exact.size else 0.0
        r = dict(exact=exact, scale=scale, rc=rc, K=K, roundings=0, pre=None, factor=None)
        if hpre:
            r["factor"] = np.where(d["hpre"] > 0, np.float32(1.0), np.float32(SLOPE)).astype(np.float32)
            r["roundings"] = (r["factor"] != 1).astype(np.float64)             # the multiply by the slope
        if prefill:
            rng = np.random.default_rng(zlib.crc32((base + name).encode()))
            r["pre"] = (rng.standard_normal(exact.shape) * (np.median(scale) / 16)).astype(np.float32)
            r["roundings"] = float(-(-K // 128)) if c["kind"] == "grad_x_res" else 1.0    # one add per launch that adds into it
        want, sc = exact, scale
        if r["factor"] is not None:
            want, sc = exact * r["factor"], scale * r["factor"]
        if r["pre"] is not None:
            want = want + r["pre"]
        r["want"], r["wscale"] = want, sc
        ref[name] = r
    return ref


def reference(c):
    return _reference(c["base"], c["hpre"], c["prefill"])


def finish(c, name, v):
    """what the kernel's epilogue makes of the fp32 product v of output `name` (numpy models of kernels: the CPU tests)"""
    r = reference(c)[name]
    if r["factor"] is not None:
        v = (v * r["factor"]).astype(np.float32)
    if r["pre"] is not None:
        v = (r["pre"] + v).astype(np.float32)
    return v


def judge(c, env, outputs, record=None):
    """outputs {name: fp32 array} against the case's reference -> (records, failures).  A record: ratio, rc, bound, share."""
    recs, bad = {}, []
    for name, r in reference(c).items():
        got = np.asarray(outputs[name], np.float32).reshape(r["want"].shape)
        ratio = R.ratio_with_rounding(got, r["want"], r["wscale"], r["roundings"])
        if not np.all(np.isfinite(got)):
            ratio = float("inf")
        rc, K = r["rc"], r["K"]
        bound = R.chain_bound(rc)
        rec = dict(ratio=ratio, rc=rc, K=K, chain_bound=bound)
        if absolute_part_applies(c, env):
            if rc <= R.abs_bound(K):
                bound = min(bound, R.abs_bound(K))
                rec["abs_bound"] = R.abs_bound(K)
            else:
                rec["chain_misses_abs_bound"] = R.abs_bound(K)       # held to the chain-relative part alone
        rec["share"] = ratio / bound
        recs[name] = rec
        if not ratio <= bound:
            bad.append(f"{c['id']} {name}: error {ratio:.3g} x sum|a||b| above {bound:.3g} (fp32 fma chain {rc:.3g}, K = {K})")
    return recs, bad


# ---- one case on the GPU -------------------------------------------------------------------------------------------------------------
def _pad_rows(x, ldx):
    out = np.zeros((x.shape[0], ldx), np.float32)
    out[:, :x.shape[1]] = x
    return out


def _dev(torch, a, unaligned=False):
    """a device copy; unaligned: behind one leading float, so that its address is 4 bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), a]) if unaligned else a).to("cuda:0")
    t.ptr = t.data_ptr() + (4 if unaligned else 0)
    assert (t.ptr % 16 != 0) == bool(unaligned)
    return t


def run_case(A, torch, c, env):
    """-> dict(records, failures, picked, sha).  Every buffer a launch may write stands between guard bands; every cell it has no
    business writing must come back bit-identical."""
    d, ref = inputs(c["base"]), reference(c)
    kind, M, F, HD, part, ldx = c["kind"], c["M"], c["F"], c["HD"], c["part"], _ldx(c)
    G = functools.partial(R.Guarded, torch)
    bad, out, extra = [], {}, {}

    def check_guards(**bufs):
        for nm, b in bufs.items():
            if not b.words()[1]:
                bad.append(f"{c['id']}: the launch wrote into the guard band of {nm}")

    if kind == "project":
        x, W = _dev(torch, _pad_rows(d["x"], ldx), c["unaligned"]), _dev(torch, d["W"])
        cap = scratch_floats(c, env)
        stated = A.op_dense_scratch_floats(A.DENSE_SCRATCH_PROJECT, M, F, HD, part)
        if stated != project_slab_floats(M, F, HD, part, env):
            bad.append(f"{c['id']}: the library states {stated} scratch floats, the host rules {project_slab_floats(M, F, HD, part, env)}")
        runs = {}
        for bf in ((0, 1) if c["bf16"] else (0,)):
            pl = G(M * HD // 2 if bf else M * HD)
            pr, scr = G(M * HD), G(cap)
            picked = A.op_dense_project(x.ptr, c["ldx"], W.ptr, M, F, HD, part, bool(bf), pl.ptr, pr.ptr,
                                        scr.ptr if c["scratch"] != "none" else 0, cap)
            check_guards(PL=pl, PR=pr, scratch=scr)
            if part == LEFT and not pr.untouched():
                bad.append(f"{c['id']}: kPartLeft wrote into PR")
            if part == RIGHT and not pl.untouched():
                bad.append(f"{c['id']}: kPartRight wrote into PL")
            if c["scratch"] == "short" and not scr.untouched():
                bad.append(f"{c['id']}: a scratch one float short was written")
            runs[bf] = (pl.words()[0], pr.words()[0], picked)
        picked = runs[0][2]
        if part != RIGHT:
            out["PL"] = runs[0][0].view(np.float32)
        if part != LEFT:
            out["PR"] = runs[0][1].view(np.float32)
        if c["bf16"]:
            assert (M * HD) % 2 == 0
            if runs[1][2] != picked:
                bad.append(f"{c['id']}: pl_bf16 = 1 picked {runs[1][2]}, pl_bf16 = 0 {picked}")
            if part != RIGHT:
                want = (R.bf16_rne(runs[0][0].view(np.float32)).view(np.uint32) >> 16).astype(np.uint16)
                if not np.array_equal(runs[1][0].view(np.uint16), want):
                    bad.append(f"{c['id']}: the bf16 PL is not bf16_rne of the fp32 PL of the same launch, bit for bit")
            if not np.array_equal(runs[1][1], runs[0][1]):
                bad.append(f"{c['id']}: PR differs between pl_bf16 = 0 and 1")
    elif kind == "grad_x":
        gpl, gpr, W = _dev(torch, d["gpl"]), _dev(torch, d["gpr"], c["unaligned"]), _dev(torch, d["W"])
        plain = G(M * F)
        picked = A.op_dense_grad_x(gpl.ptr, gpr.ptr, W.ptr, 0, plain.ptr, M, F, HD, SLOPE)
        check_guards(gprev=plain)
        out["gprev"] = plain.words()[0].view(np.float32)
        if c["hpre"]:
            h, withh = _dev(torch, d["hpre"]), G(M * F)
            picked = A.op_dense_grad_x(gpl.ptr, gpr.ptr, W.ptr, h.ptr, withh.ptr, M, F, HD, SLOPE)
            check_guards(gprev=withh)
            got = withh.words()[0].view(np.float32)
            # the decisions, exact: the same sums (same kernel arithmetic, another epilogue) times 1 where hpre_prev > 0, else the slope
            want = (out["gprev"].reshape(M, F) * ref["gprev"]["factor"]).astype(np.float32)
            if not np.array_equal(got.view(np.int32), want.reshape(-1).view(np.int32)):
                rows = np.unique(np.nonzero(got.reshape(M, F).view(np.int32) != want.view(np.int32))[0])[:8]
                bad.append(f"{c['id']}: LReLU' decisions differ from (hpre_prev > 0 ? 1 : slope) in rows {rows.tolist()}")
            out["gprev"] = got
    elif kind in GRADW:
        gpl, gpr, x = _dev(torch, d["gpl"]), _dev(torch, d["gpr"]), _dev(torch, _pad_rows(d["x"], ldx), c["unaligned"])
        need = A.op_dense_scratch_floats(A.DENSE_SCRATCH_GRAD_W, M, F, HD)
        extra["scratch_floats"] = need
        scr = G(need)
        if kind == "grad_w":
            fill = np.zeros((HD, 2 * F), np.float32)
            if "L" in ref and ref["L"]["pre"] is not None:
                fill[:, :F] = ref["L"]["pre"]
            if "R" in ref and ref["R"]["pre"] is not None:
                fill[:, F:] = ref["R"]["pre"]
            if part == LEFT:
                fill[:, F:] = 3.25            # cells of the half the launch does not own
            if part == RIGHT:
                fill[:, :F] = 3.25
            gw = G(HD * 2 * F, fill)
            picked = A.op_dense_grad_w(gpl.ptr if part != RIGHT else 0, gpr.ptr if part != LEFT else 0, x.ptr, c["ldx"],
                                       gw.ptr, scr.ptr, need, M, F, HD, part)
            got = gw.words()[0].view(np.float32).reshape(HD, 2 * F)
            if part != RIGHT:
                out["L"] = got[:, :F]
            elif not np.array_equal(got[:, :F], fill[:, :F]):
                bad.append(f"{c['id']}: kPartRight wrote into the left columns of gradW")
            if part != LEFT:
                out["R"] = got[:, F:]
            elif not np.array_equal(got[:, F:], fill[:, F:]):
                bad.append(f"{c['id']}: kPartLeft wrote into the right columns of gradW")
        else:
            gw = G(HD * F, ref["gradWres"]["pre"])
            picked = A.op_dense_grad_wres(gpl.ptr, x.ptr, c["ldx"], gw.ptr, scr.ptr, need, M, F, HD)
            out["gradWres"] = gw.words()[0].view(np.float32)
        check_guards(gradW=gw, scratch=scr)
    elif kind == "project_res":
        x, W, r = _dev(torch, _pad_rows(d["x"], ldx)), _dev(torch, d["Wres"]), G(M * HD)
        picked = A.op_dense_project_res(x.ptr, c["ldx"], W.ptr, r.ptr, M, F, HD)
        check_guards(R=r)
        out["R"] = r.words()[0].view(np.float32)
    else:
        g, W, gx = _dev(torch, d["g"]), _dev(torch, d["Wres"]), G(M * F, ref["gx"]["pre"])
        picked = A.op_dense_grad_x_res(g.ptr, W.ptr, gx.ptr, M, F, HD)
        check_guards(gx=gx)
        out["gx"] = gx.words()[0].view(np.float32)
    if picked != pick(c, env):
        bad.append(f"{c['id']}: the launcher picked {picked}, the host rules say {pick(c, env)}")
    recs, fails = judge(c, env, out)
    sha = hashlib.sha1(b"".join(np.ascontiguousarray(out[k]).tobytes() for k in sorted(out))).hexdigest()
    return dict(records=recs, failures=bad + fails, picked=picked, sha=sha, **extra)


def record_case(parity, c, tag, res):
    for name, rec in res["records"].items():
        parity.record(f"{tag} | {c['id']} | {name}", rec["ratio"], rec.get("abs_bound", rec["chain_bound"]), fp32_fma_chain=rec["rc"],
                      share=rec["share"], picked=res["picked"], K=rec["K"],
                      **({"chain_misses_abs_bound": rec["chain_misses_abs_bound"]} if "chain_misses_abs_bound" in rec else {}))


def run_setting(pkg, tag):
    """Every case of one switch setting in this process (the switches are read once per process).  Prints one RESULT line per case and
    raises at the end with every failure; -> number of cases."""
    import torch
    import parity
    env, _ = SETTING[tag]
    parity.set_test(f"tests/test_dense_seams.py::setting[{tag}]")
    failures, n = [], 0
    for c in cases_of(tag):
        res = run_case(pkg.abi, torch, c, env)
        record_case(parity, c, tag, res)
        print("RESULT", json.dumps(dict(id=c["id"], picked=res["picked"], sha=res["sha"], failures=res["failures"],
                                        records={k: {q: v[q] for q in ("ratio", "rc", "share")} for k, v in res["records"].items()})))
        failures += res["failures"]
        n += 1
    parity.flush()
    assert not failures, "\n".join(failures)
    return n
