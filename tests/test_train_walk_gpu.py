"""The training programs walked ONE OP AT A TIME on a real MI355X next to the float64 reference of every op
(tests/train_ref.py): only the launches the lowering itself emits, with the arguments it emits -- in-place accumulation
(acc_in == dx, aux == dst), the reduction scratch inside the zero-filled gradient arena (EAB_NB_SUMS_ZEROED), the weight
gradients as the batched run eab_run_program makes of them.

Per case: parameters with random PReLU slopes are packed by the program's own gather launch (checked bit for bit against
the index tables), the activation arena is NaN-filled, the gradient arena zero-filled.  Then for every op of the forward and
the backward list: the regions it reads are copied to the host, the op runs alone, and
  * the set of changed words of the arenas (compared as int32 on the device) lies inside the op's outputs and declared
    scratch; the packed weights and the boundary inputs never change;
  * every element the op must write is finite (the arena was NaN);
  * the outputs meet the derived per-element limit and, per output region, an L2-relative error of at most conv_ref.MARGIN
    times that of the fp32 yardstick evaluation (both against float64).  The LSTM recurrences keep their 1e-5 bar; the
    double-precision scratch of the cLN ops is compared as doubles.
The device's own outputs stay in the arena: errors do not compound, and every op sees the activations and gradients a
training step really produces.  Every maximal run of weight gradients is run twice from the same state of the gradient
arena: as one eab_run_program call (batched launches) and one call per op; both must meet the limits.  At the end the
flat gradient of the program's inverse gather is checked bit for bit."""
import time

import numpy as np
import pytest
import torch

import conv_ref as cr
import train_ref as tref
from eabnet_amd import program as prg
from eabnet_amd import train as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from eabnet_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Walk:
    def __init__(self, case: tref.Case, dev):
        self.case, self.dev = case, dev
        prog = case.prog
        self.bound = b = tr.TrainBound(prog, dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.flat = torch.from_numpy(case.flat).to(dev)
        b.pack(self.flat, self.stream)
        b.acts.fill_(float("nan"))
        b.g.zero_()
        self.io = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in case.boundary.items()}
        b.use_graph = False
        b.bind(*(self.io[k].data_ptr() if k in self.io else None for k in b.BOUNDARY))
        self.arena = {"a": b.acts, "w": b.w, "g": b.g, **{k: v.view(-1) for k, v in self.io.items()}}
        self.mutable = ["a", "g", "out"]
        self.pristine = {k: self.arena[k].clone() for k in ("w", "in", "in2", "dout") if k in self.arena}
        torch.cuda.synchronize()
        self.stats = {}                     # kind -> [ops, worst err / limit, worst L2 ratio, ambiguous, elements that can be]

    # -- pieces ----------------------------------------------------------------------------------------------------
    def fetch(self, a: tref.Access) -> np.ndarray:
        v = self.arena[a.ref.arena][a.ref.off:a.ref.off + a.words].cpu().numpy()
        return (v.view(np.float64) if a.dtype == "f64" else v).reshape(a.shape)

    def region(self, o: tref.Out) -> np.ndarray:
        words = int(np.prod(o.shape)) * (2 if o.f64 else 1)
        v = self.arena[o.ref.arena][o.ref.off:o.ref.off + words].cpu().numpy()
        return (v.view(np.float64) if o.f64 else v).reshape(o.shape)

    def snapshot(self):
        return {k: self.arena[k].clone() for k in self.mutable}

    def changed_only(self, before, outs, what):
        """the words that differ from ``before`` lie inside the may sets of ``outs``; nothing else of the machine changed"""
        flags = []
        for k in self.mutable:
            ch = self.arena[k].view(torch.int32) != before[k].view(torch.int32)
            for o in outs:
                if o.ref.arena != k:
                    continue
                words = int(np.prod(o.shape)) * (2 if o.f64 else 1)
                sl = slice(o.ref.off, o.ref.off + words)
                if o.may.all():
                    ch[sl] = False
                else:
                    may = np.repeat(o.may.reshape(-1), 2) if o.f64 else o.may.reshape(-1)
                    ch[sl] &= ~torch.from_numpy(np.ascontiguousarray(may)).to(self.dev)
            flags.append(ch.any())
        for k, t in self.pristine.items():
            flags.append((self.arena[k].view(torch.int32) != t.view(torch.int32)).any())
        flags = torch.stack(flags).cpu().numpy()
        names = self.mutable + list(self.pristine)
        bad = [n for n, f in zip(names, flags) if f]
        assert not bad, f"{what}: words changed outside the op's outputs and declared scratch, in arena(s) {bad}"

    def note(self, kind, worst, l2, amb=0, elems=0):
        s = self.stats.setdefault(kind, [0, 0.0, None, 0, 0])
        s[0] += 1
        s[1] = max(s[1], worst)
        if l2 is not None:
            s[2] = l2 if s[2] is None else max(s[2], l2)
        s[3] += amb
        s[4] += elems

    # -- one op ----------------------------------------------------------------------------------------------------
    def step(self, lst: str, k: int, op):
        what = f"{self.case.name} {lst}[{k}] {op.name} ({tref.kind_name(op)})"
        outs, amb = tref.evaluate(op, self.fetch)
        lstm = op.kind in (tr.OP_LSTM_TRAIN, tr.OP_LSTM_BWD)
        yard = None if lstm else {n: o.val for n, o in tref.evaluate(op, self.fetch, np.float32)[0].items()}
        before = self.snapshot()
        self.bound.run(lst, self.stream, k, 1)
        torch.cuda.synchronize()
        self.changed_only(before, list(outs.values()), what)
        got = {n: self.region(o) for n, o in outs.items()}
        worst, l2 = tref.check(outs, got, yard, what, l2_names=cr.L2_NAMES if op.kind == prg.OP_CONV else None)
        kink = op.kind in (tr.OP_NORM_BWD, tr.OP_CLN_BWD)
        self.note(tref.kind_name(op), worst, l2, amb, outs["dx"].val.size if kink else 0)

    # -- a run of weight gradients ---------------------------------------------------------------------------------
    def wgrad_run(self, lst: str, first: int, count: int):
        ops = self.bound.lists[lst][first:first + count]
        g0 = self.bound.g.clone()
        host = g0.cpu().numpy()
        v64, lim, v32 = host.astype(np.float64), np.zeros(host.size), host.copy()
        touched = {}
        m64, m32 = tref._M(np.float64), tref._M(np.float32)
        for op in ops:                      # the run in program order on float64 / fp32 shadows of the gradient arena
            A = {a.name: self.fetch(a) for a in tref.accesses(op) if a.mode == "r"}
            with np.errstate(over="ignore", invalid="ignore"):
                t64, t32 = tref.wgrad_terms(op, A, m64), tref.wgrad_terms(op, A, m32)
            R = op.B * op.T * op.No
            for ref, n, d64, l, d32 in ((op.dw, op.N * op.Kpad, t64[0], t64[1], t32[0]), (op.dbias, op.N, t64[2], t64[3], t32[2])):
                if ref is None:
                    continue
                assert ref.arena == "g"
                sl = slice(ref.off, ref.off + n)
                lim[sl] += tref.SECOND * (l.reshape(-1) + (R + 2) * tref.U * np.abs(v64[sl]))
                v64[sl] += d64.reshape(-1)
                v32[sl] = v32[sl] + d32.reshape(-1).astype(np.float32)
                touched[(ref.off, n)] = ref
        outs = {f"g+{off}": tref.Out(ref, (n,), v64[off:off + n], lim[off:off + n], np.ones(n, bool), np.ones(n, bool), name=f"g+{off}")
                for (off, n), ref in touched.items()}
        yard = {name: v32[o.ref.off:o.ref.off + o.shape[0]] for name, o in outs.items()}
        for how, calls in (("one call", [(first, count)]), ("one call per op", [(first + j, 1) for j in range(count)])):
            what = f"{self.case.name} {lst}[{first}:{first + count}] {count} weight gradients, {how} ({ops[0].name} ...)"
            self.bound.g.copy_(g0)
            before = self.snapshot()
            for f, n in calls:
                self.bound.run(lst, self.stream, f, n)
            torch.cuda.synchronize()
            self.changed_only(before, list(outs.values()), what)
            got = {n: self.region(o) for n, o in outs.items()}
            try:
                worst, l2 = tref.check(outs, got, yard, what)
            except AssertionError as e:         # name the op whose dw / dbias it is
                owner = [o.name for o in ops if any(f" g+{r.off}:" in str(e) for r in (o.dw, o.dbias) if r is not None)]
                raise AssertionError(f"{e}  [{', '.join(owner)}]") from None
            self.note("WGRAD" if how == "one call" else "WGRAD (single)", worst, l2)
            self.stats["WGRAD" if how == "one call" else "WGRAD (single)"][0] += count - 1

    # -- everything ------------------------------------------------------------------------------------------------
    def run(self):
        prog, b = self.case.prog, self.bound
        # the gather launch: packed[i] = flat[ia[i]] (+ flat[ib[i]]), a negative index contributes 0
        flat, ia, ib = self.case.flat, prog.ia, prog.ib
        want = np.where(ia >= 0, flat[ia], np.float32(0))
        if ib is not None:
            want = np.where(ib >= 0, want + flat[ib], want)
        packed = b.w[:prog.w_floats].cpu().numpy()
        assert np.array_equal(packed.view(np.int32), want.astype(np.float32).view(np.int32)), "eab_gather_f32: packed arena != flat[ia] (+ flat[ib])"
        for lst in ("fwd", "bwd"):
            ops = b.lists[lst]
            runs = dict(tref.wgrad_runs(ops))
            k = 0
            while k < len(ops):
                if k in runs:
                    self.wgrad_run(lst, k, runs[k])
                    k += runs[k]
                else:
                    self.step(lst, k, ops[k])
                    k += 1
        # the inverse gather: flat gradient = g[inv], parameters without an entry get 0
        gflat = torch.full((prog.n_params,), float("nan"), device=self.dev)
        b.unpack_grads(gflat, self.stream)
        torch.cuda.synchronize()
        g = b.g.cpu().numpy()
        want = np.where(prog.inv >= 0, g[prog.inv], np.float32(0))
        assert np.array_equal(gflat.cpu().numpy().view(np.int32), want.view(np.int32)), "eab_gather_f32 (gradients): flat gradient != g[inv]"
        assert np.isfinite(self.io["out"].cpu().numpy()).all()


@pytest.mark.parametrize("name", list(tref.CASES))
def test_every_training_op_matches_float64(dev, name):
    t0 = time.time()
    case = tref.make_case(name)
    walk = Walk(case, dev)
    walk.run()
    amb = sum(s[3] for s in walk.stats.values())
    elems = sum(s[4] for s in walk.stats.values())
    print()
    for kind, (n, worst, l2, a, _) in sorted(walk.stats.items()):
        print(f"WALK {name} | {kind} | {n} ops | err/limit {worst:.3f} | L2 ratio {'-' if l2 is None else format(l2, '.2f')} | ambiguous {a}")
    print(f"WALK {name} | {len(case.prog.fwd)} + {len(case.prog.bwd)} ops | ambiguous {amb} of {elems} (cap {tref.KINK_CAP:g}) | {time.time() - t0:.1f} s")
    assert amb <= tref.KINK_CAP * elems, f"{amb} of {elems} elements lie on the PReLU kink: pick another seed"
