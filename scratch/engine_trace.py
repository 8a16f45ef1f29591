"""Launch trace of the engine's host side on the CPU, for comparing two trees of this repository call for call
(profiles/engine_refactor_equivalence.md).  tests/fakelib.py replaces the C ABI by a recorder; here every call records its
symbol, every integer / float argument, every field of a by-reference struct (addresses as null / non-null) and, for every
tensor pointer, dtype, element count, storage offset and storage size, plus which pointer arguments of the call share an
address.  Interleaved with the calls: every engine workspace request (key, size, dtype), every torch.empty / zeros / empty_like /
zeros_like (allocation order) and every gradient-ready notification.

    python scratch/engine_trace.py TREE_A TREE_B [--md FILE]     compare two trees (each traced in its own process; a
                                                                 directory written by --dump stands for its tree)
    python scratch/engine_trace.py --dump TREE OUTDIR           one trace file per configuration + index.json
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

SWITCHES = ("SM3_LINBN_FWD", "SM3_LINBN_DS", "SM3_LINBN_JOIN", "SM3_LINBN_MERGE", "SM3_LANE_CROSS")
ENV = SWITCHES + ("SM3_LINBN", "SM3_WGRAD_DET", "SM3_STEM16", "SM3_PAIR_VIEWS")


def _configs():
    """(name, function, environment) triples."""
    import torch
    from src.models import resnet
    from src.models.simclr import SimCLR, SimCLRSkinV3, SimCLRSkinV32
    from sm3hip.engine import SM3Engine
    from sm3hip.trainer import SM3Trainer
    dts = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

    def imgs(B, n=4, S=32):
        g = torch.Generator().manual_seed(0)
        return [torch.randn(B, 3, S, S, generator=g) for _ in range(n)]

    def trainer_steps(model, dt, B, steps=2, setup=None, meta=None, **kw):
        model.sm3_dtype = dts[dt]
        tr = SM3Trainer(model, lr=1e-3, data_parallel=False, **kw)
        eng = tr._engine()
        if setup is not None:
            setup(eng)
        x = imgs(B)
        for _ in range(steps):
            tr.step(x[:2], x[2:], metadata=meta)

    def sync_stub(eng):
        eng.stat_sync, eng.world_size = (lambda t: None), 2
        setattr(eng, "_explicit_sync", True)

    out = []
    add = lambda name, fn, **env: out.append((name, fn, env))
    v32 = lambda arch="resnet50", **kw: SimCLRSkinV32(arch, None, 128, 0.1, **kw)
    for dt in dts:
        for B in (2, 128):
            add(f"v32 resnet50 {dt} B={B}", lambda dt=dt, B=B: trainer_steps(v32(), dt, B))
    for arch in ("resnet18", "resnet34", "resnext50_32x4d"):
        for B in (2, 128):
            add(f"v32 {arch} bf16 B={B}", lambda arch=arch, B=B: trainer_steps(v32(arch), "bf16", B))
    add("v32 resnext50_32x4d f32 B=2", lambda: trainer_steps(v32("resnext50_32x4d"), "f32", 2))
    add("v32 resnet18 f32 B=2", lambda: trainer_steps(v32("resnet18"), "f32", 2))
    for B in (2, 128):
        add(f"v3 resnet50 bf16 B={B}", lambda B=B: trainer_steps(SimCLRSkinV3("resnet50", None, 128, 0.1), "bf16", B))
    add("v32 resnet50 bf16 B=128 SM3_PAIR_VIEWS=0", lambda: trainer_steps(v32(), "bf16", 128), SM3_PAIR_VIEWS="0")
    add("v32 resnet50 bf16 B=128 two_streams off",
        lambda: trainer_steps(v32(), "bf16", 128, setup=lambda e: setattr(e, "two_streams", False)))
    for sw in SWITCHES + ("SM3_LINBN", "SM3_WGRAD_DET", "SM3_STEM16"):
        for B in (2, 128):
            add(f"v32 resnet50 bf16 B={B} {sw}=0", lambda B=B: trainer_steps(v32(), "bf16", B), **{sw: "0"})
    add("v32 resnet50 f16 B=2 SM3_LINBN_DS=0 SM3_LINBN_JOIN=0", lambda: trainer_steps(v32(), "f16", 2),
        SM3_LINBN_DS="0", SM3_LINBN_JOIN="0")
    add("v32 resnet50 bf16 B=2 SM3_LINBN_FWD=0 SM3_LINBN_DS=0", lambda: trainer_steps(v32(), "bf16", 2),
        SM3_LINBN_DS="0", SM3_LINBN_FWD="0")
    for extra, env in (("", {}), (" SM3_LINBN_JOIN=0", {"SM3_LINBN_JOIN": "0"}), (" SM3_LINBN_DS=0", {"SM3_LINBN_DS": "0"}),
                       (" SM3_LINBN_FWD=0", {"SM3_LINBN_FWD": "0"}), (" SM3_LINBN=0", {"SM3_LINBN": "0"})):
        for B in (2, 128):
            add(f"v32 resnet50 bf16 B={B} stat_sync world 2{extra}",
                lambda B=B: trainer_steps(v32(), "bf16", B, setup=sync_stub), **env)
    add("v32 resnet18 bf16 B=2 stat_sync world 2", lambda: trainer_steps(v32("resnet18"), "bf16", 2, setup=sync_stub))
    add("v32 resnet50 f32 B=2 stat_sync world 2", lambda: trainer_steps(v32(), "f32", 2, setup=sync_stub))
    add("v32 resnet50 bf16 B=2 target momentum", lambda: trainer_steps(v32(), "bf16", 2, target_momentum=0.99))
    add("v32 resnet50 bf16 B=128 target momentum", lambda: trainer_steps(v32(), "bf16", 128, target_momentum=0.99))
    add("v32 resnet50 bf16 B=2 metadata",
        lambda: trainer_steps(v32(metadata_dim=20), "bf16", 2, meta=torch.ones(2, 20)))
    for style in (1, 2):
        add(f"v32 resnet50 bf16 B=2 style {style}", lambda style=style: trainer_steps(v32(), "bf16", 2, style=style))

    def engine_model(kind, dt, B, train=True, want_grad=True, want_dx=None, params=True, dfeat=False, arch="resnet50"):
        """forward / backward of the engine itself (kinds the trainer does not drive, and the options of backward)."""
        model = {"v32": lambda: v32(arch), "v3": lambda: SimCLRSkinV3(arch, None, 128, 0.1),
                 "simclr": lambda: SimCLR(arch, None, 128, 0.1)}[kind]()
        model.train(train)
        eng = SM3Engine(model, dts[dt], kind)
        x = imgs(B)
        views = {"main": x[:2]} if kind == "simclr" else {"derm": x[:2], "clinic": x[2:]}
        for _ in range(2):
            zs, feats, saved = eng.forward(views, 0, train, want_grad)
            if not want_grad:
                continue
            dz = {k: torch.zeros(z.shape, dtype=dts[dt]) for k, z in zs.items()}
            df = {k: torch.zeros(f[1].shape, dtype=dts[dt]) for k, f in feats.items()} if dfeat else None
            if dfeat:
                dz.pop(next(iter(views)))  # one branch: gradient through the pooled features alone
            eng.store.flat_g.zero_()
            eng.backward(saved, dz, dfeat=df, want_dx=want_dx, params=params)

    for dt in ("bf16", "f32"):
        add(f"simclr resnet50 {dt} B=2", lambda dt=dt: engine_model("simclr", dt, 2))
    add("simclr resnet50 bf16 B=128", lambda: engine_model("simclr", "bf16", 128))
    add("simclr resnet18 bf16 B=2", lambda: engine_model("simclr", "bf16", 2, arch="resnet18"))
    add("v32 resnet50 bf16 B=2 eval want_grad", lambda: engine_model("v32", "bf16", 2, train=False))
    add("v32 resnet18 bf16 B=2 eval want_grad", lambda: engine_model("v32", "bf16", 2, train=False, arch="resnet18"))
    add("v32 resnet50 f32 B=2 eval want_grad", lambda: engine_model("v32", "f32", 2, train=False))
    add("v32 resnet50 bf16 B=2 inference", lambda: engine_model("v32", "bf16", 2, train=False, want_grad=False))
    add("v32 resnext50_32x4d bf16 B=2 inference",
        lambda: engine_model("v32", "bf16", 2, train=False, want_grad=False, arch="resnext50_32x4d"))
    add("v32 resnet50 bf16 B=2 train no grad", lambda: engine_model("v32", "bf16", 2, want_grad=False))
    for B in (2, 128):
        add(f"v32 resnet50 bf16 B={B} want_dx",
            lambda B=B: engine_model("v32", "bf16", B, want_dx={"derm": (True, False), "clinic": (True, True)}))
    add("v32 resnet50 bf16 B=2 want_dx data-only",
        lambda: engine_model("v32", "bf16", 2, want_dx={"derm": (True, True)}, params=False))
    add("v32 resnet50 bf16 B=2 dfeat", lambda: engine_model("v32", "bf16", 2, dfeat=True))
    add("v3 resnet50 bf16 B=2 engine", lambda: engine_model("v3", "bf16", 2))

    def encoder(arch, dt, B, train, keep=None, stop_at=None, params=True, dx=False, sync=False):
        mod = getattr(resnet, arch)(weights=None)
        mod.train(train)
        eng = SM3Engine(mod, dts[dt], "encoder")
        if sync:
            sync_stub(eng)
        x = imgs(B, 1)[0]
        for _ in range(2):
            k = {"stage": keep} if keep else None
            f32, ctx = eng.encoder_only("main", x, train, True, keep=k)
            eng.store.flat_g.zero_()
            dxo = torch.empty_like(x) if dx else None
            eng.encoder_backward(ctx, torch.zeros(f32.shape, dtype=dts[dt]), dx_out=dxo, params=params, stop_at=stop_at)
            eng.encoder_only("main", x, train, False, keep=k)

    for arch in ("resnet50", "resnet18", "resnet34", "resnext50_32x4d"):
        for dt in ("bf16", "f32"):
            add(f"encoder {arch} {dt} B=2 train", lambda arch=arch, dt=dt: encoder(arch, dt, 2, True))
            add(f"encoder {arch} {dt} B=2 eval keep=layer3 stop_at=layer2 data-only dx_out",
                lambda arch=arch, dt=dt: encoder(arch, dt, 2, False, keep="layer3", stop_at="layer2", params=False))
        add(f"encoder {arch} bf16 B=2 eval stop_at=layer3 data-only",
            lambda arch=arch: encoder(arch, "bf16", 2, False, stop_at="layer3", params=False))
        add(f"encoder {arch} bf16 B=2 eval dx_out data-only",
            lambda arch=arch: encoder(arch, "bf16", 2, False, params=False, dx=True))
        add(f"encoder {arch} bf16 B=2 train dx_out", lambda arch=arch: encoder(arch, "bf16", 2, True, dx=True))
    add("encoder resnet50 f16 B=128 train", lambda: encoder("resnet50", "f16", 128, True))
    add("encoder resnet50 bf16 B=2 train stat_sync world 2", lambda: encoder("resnet50", "bf16", 2, True, sync=True))
    add("encoder resnet50 bf16 B=2 eval stat_sync world 2", lambda: encoder("resnet50", "bf16", 2, False, sync=True))
    return out


class _Trace:
    lines = []


T = _Trace()


def dump(tree, outdir):
    sys.path[:0] = [os.path.join(tree, "skin-sm3_amd"), os.path.join(tree, "tests")]
    import torch
    import fakelib
    from sm3hip import ops
    from sm3hip.engine import SM3Engine
    os.makedirs(outdir, exist_ok=True)
    torch.manual_seed(0)

    class Ptr(C.c_void_p):
        pass

    def ptr(t):
        p = Ptr(0 if t is None else t.data_ptr())
        if t is not None:
            p.info = (str(t.dtype), t.numel(), t.storage_offset(), t.untyped_storage().nbytes())
        return p
    ops._ptr = ptr

    def val(a, addrs):
        if a is None:
            return "None"
        if isinstance(a, Ptr):
            if not a.value:
                return "null"
            first = addrs.setdefault(a.value, len(addrs))
            return f"ptr{first}{a.info}"
        if isinstance(a, C.c_void_p):
            return "nonnull" if a.value else "null"
        if hasattr(a, "_obj"):  # byref
            return val(a._obj, addrs)
        if isinstance(a, C.Structure):
            return type(a).__name__ + "{" + ",".join(
                f"{n}={('nonnull' if getattr(a, n) else 'null') if ct is C.c_void_p else val(getattr(a, n), addrs)}"
                for n, ct in a._fields_) + "}"
        if isinstance(a, C.Array):
            return "[" + ",".join(val(x, addrs) for x in a) + "]"
        if isinstance(a, C._SimpleCData):
            return repr(a.value)
        if isinstance(a, (bool, int, float, str)):
            return repr(a)
        if isinstance(a, torch.Tensor):
            return f"tensor({a.dtype},{a.numel()})"
        return type(a).__name__

    def fake_call(self, *args):
        addrs = {}
        T.lines.append(self.name + "(" + ", ".join(val(a, addrs) for a in args) + ")")
        return orig_call(self, *args)
    orig_call = fakelib._FakeFn.__call__
    fakelib._FakeFn.__call__ = fake_call

    orig_work = SM3Engine._work

    def work(self, key, numel, dtype=torch.float32):
        T.lines.append(f"WORK {self._lane}/{key} {numel} {dtype}")
        return orig_work(self, key, numel, dtype)
    SM3Engine._work = work
    orig_notify = SM3Engine._notify

    def notify(self, first, last):
        seen = []
        gr = self.grad_ready
        if gr is not None:
            self.grad_ready = lambda f, l: (seen.append((f, l)), gr(f, l))
        try:
            orig_notify(self, first, last)
        finally:
            self.grad_ready = gr
        T.lines.append(f"NOTIFY {first} {last} delivered={seen}")
    SM3Engine._notify = notify

    # allocation order of the engine (and of everything else that allocates through torch while a configuration runs)
    def traced(name, fn):
        def f(*a, **k):
            t = fn(*a, **k)
            T.lines.append(f"ALLOC {name} {tuple(t.shape)} {t.dtype}")
            return t
        return f
    for name in ("empty", "zeros", "empty_like", "zeros_like"):
        setattr(torch, name, traced(name, getattr(torch, name)))

    index = {}
    for name, fn, env in _configs():
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)
        T.lines = []
        with fakelib.installed():
            ops._ptr = ptr
            try:
                fn()
            except Exception as e:  # a configuration the tree refuses: both trees must refuse it alike
                T.lines.append(f"RAISED {type(e).__name__}: {e}")
        text = "\n".join(T.lines) + "\n"
        fname = hashlib.sha1(name.encode()).hexdigest()[:12] + ".txt"
        with open(os.path.join(outdir, fname), "w") as f:
            f.write(text)
        index[name] = {"file": fname, "calls": sum(1 for l in T.lines if l.startswith("sm3_")), "lines": len(T.lines),
                       "sha1": hashlib.sha1(text.encode()).hexdigest(),
                       "raised": next((l for l in T.lines if l.startswith("RAISED")), None)}
        print(f"{index[name]['calls']:7d} {index[name]['sha1'][:10]} {name}" + (f"   {index[name]['raised']}" if index[name]["raised"] else ""), flush=True)
    with open(os.path.join(outdir, "index.json"), "w") as f:
        json.dump(index, f, indent=1)


def compare(a, b, md):
    import tempfile
    tmp = tempfile.mkdtemp(prefix="engine_trace_")
    dirs = []
    for i, tree in enumerate((a, b)):
        d = os.path.join(tmp, "ab"[i])
        if os.path.exists(os.path.join(tree, "index.json")):  # a directory written by --dump earlier
            dirs.append(tree)
            continue
        subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", os.path.abspath(tree), d], check=True,
                       stdout=subprocess.DEVNULL)
        dirs.append(d)
    ia, ib = (json.load(open(os.path.join(d, "index.json"))) for d in dirs)
    rows, bad = [], 0
    for name in ia:
        ra, rb = ia[name], ib.get(name)
        if rb is not None and ra["sha1"] == rb["sha1"]:
            res = "equal" if not ra["raised"] else "equal (both raise: " + ra["raised"][7:60] + ")"
        else:
            bad += 1
            la = open(os.path.join(dirs[0], ra["file"])).read().split("\n")
            lb = open(os.path.join(dirs[1], rb["file"])).read().split("\n") if rb else []
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            res = f"DIFFERENT at line {i}: `{(la[i] if i < len(la) else '<end>')[:120]}` / `{(lb[i] if i < len(lb) else '<end>')[:120]}`"
        rows.append(f"| {name} | {ra['calls']} | {ra['lines']} | {res} |")
    table = "\n".join(["| configuration | kernel calls | trace lines | parent against head |", "|---|---|---|---|"] + rows)
    print(table)
    print(f"\n{len(rows)} configurations, {bad} different; traces in {tmp}")
    if md:
        with open(md, "w") as f:
            f.write(table + "\n")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--dump":
        dump(sys.argv[2], sys.argv[3])
    else:
        md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
        sys.exit(1 if compare(sys.argv[1], sys.argv[2], md) else 0)
