"""The body of one child process of tests/test_gpu_linear_cfgs.py: DVM_LINEAR_CFG is read once when the library is loaded, so every
forced tile configuration needs a process of its own.  main(c, refs) runs every case of tests/linear_cfg_cases.py on the GPU with
the configuration the environment forces, compares every element with the oracle's result (made once by the parent, handed over
in the .npz file `refs`) bit for bit, and after every call compares dvm_linear_last_launch with what the route predicates say the
call must have launched.  Prints the (channel_major, index, dma) triples it saw, one SHA-256 over its point-major outputs and, only
when every comparison held, the line the parent waits for."""
import ctypes
import hashlib
import os

import numpy as np
import torch

import linear_cfg_cases as LC


def main(c, refs_path):
    from dvm import _lib, ops
    assert os.environ.get("DVM_LINEAR_CFG") == str(c)
    lib = _lib.load()
    refs = np.load(refs_path)
    seen, used, digest = set(), set(), hashlib.sha256()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731

    def last(want, what):
        info = (ctypes.c_int * 8)()
        ops.check(lib.dvm_linear_last_launch(info), "dvm_linear_last_launch")
        assert list(info) == want, "%s: dvm_linear_last_launch %s, the route predicates say %s" % (what, list(info), want)
        seen.add(tuple(info[:3]))

    def same(got, name, what):
        used.add(name)
        got, want = got.cpu().numpy(), refs[name]
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError("%s: %d of %d elements differ from the oracle, first at %s: %r, expected %r" % (
                what, len(bad), got.size, bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))
        return got

    def pm_call(d, **kw):
        return ops.linear(dev(d["x"]) if "x" not in kw else kw.pop("x"), dev(d["w"]) if "w" not in kw else kw.pop("w"),
                          bias=dev(d["bias"]), res=dev(d["res"]), bn=None if d["alpha"] is None else (dev(d["alpha"]), dev(d["beta"])),
                          slope=d["slope"], **kw)

    # ---- the point-major table
    for M, K, Co in LC.PM_CASES:
        for ep in LC.PM_EPILOGUES:
            what = "point-major M=%d K=%d Co=%d epilogue %s" % (M, K, Co, ep)
            got = pm_call(LC.pm_inputs(M, K, Co, ep))
            last(LC.expect(c, 0, M, K, Co), what)
            digest.update(same(got, "pm_%d_%d_%d_%s" % (M, K, Co, ep), what).tobytes())

    # ---- the channel-major table (c >= 4 is no entry of that table: the default applies), per batch element
    for N, K, Co in LC.CM_CASES:
        what = "channel-major N=%d K=%d Co=%d" % (N, K, Co)
        d = LC.cm_inputs(N, K, Co)
        got = ops.linear(dev(d["x"]), dev(d["w"]), bias=dev(d["bias"]), bn=(dev(d["alpha"]), dev(d["beta"])), channel_major=True)
        e = LC.expect(c, 1, None, K, Co, N=N)
        assert e[1] == (c if c < 4 else (0 if Co <= 32 else 1))
        last(e, what)
        g = got.cpu().numpy()
        for b in range(LC.CM_B):
            assert np.array_equal(g[b], refs["cm_%d_%d_%d" % (N, K, Co)][b]), "%s: batch element %d differs from the oracle" % (what, b)
        same(got, "cm_%d_%d_%d" % (N, K, Co), what)

    # ---- the row prefix against the oracle on the explicit concatenation: never a DMA launch
    for B, N, Cg, Cx, Co in LC.PREFIX_CASES:
        what = "prefix B=%d N=%d Cg=%d Cx=%d Co=%d" % (B, N, Cg, Cx, Co)
        d = LC.prefix_inputs(B, N, Cg, Cx, Co)
        got = ops.linear(dev(d["x"]), dev(d["w"]), bn=(dev(d["alpha"]), dev(d["beta"])), slope=0.2, prefix=dev(d["g"]))
        e = LC.expect(c, 0, B * N, Cg + Cx, Co, prefix=True)
        assert e[2] == 0
        last(e, what)
        same(got, "prefix_%d_%d_%d_%d_%d" % (B, N, Cg, Cx, Co), what)

    # ---- the scaled residual against plain * s + r
    for cm, (B, N, K, Co) in ((0, LC.SCALED_PM), (1, LC.SCALED_CM)):
        what = "scaled residual channel_major=%d" % cm
        d = LC.scaled_inputs(cm, B, N, K, Co)
        got = ops.linear(dev(d["x"]), dev(d["w"]), bias=dev(d["bias"]), channel_major=bool(cm), post=(LC.SCALE, dev(d["r"])))
        last(LC.expect(c, cm, B * N, K, Co, N=N), what)
        same(got, "scaled_%d" % cm, what)

    # ---- guards: `out` a contiguous view inside a buffer of sentinels, off (67 floats in) and on (64) the 16-byte grid
    for M, K, Co in LC.GUARD_CASES:
        for ep in LC.PM_EPILOGUES:
            for lead, yv in LC.GUARD_OFFSETS.items():
                what = "guards M=%d K=%d Co=%d epilogue %s, out %d floats in" % (M, K, Co, ep, lead)
                n = M * Co
                big = torch.full((lead + n + LC.GUARD_PAD,), LC.SENTINEL, dtype=torch.float32, device="cuda")
                out = big[lead:lead + n].view(M, Co)
                assert out.is_contiguous() and (out.data_ptr() % 16 == 0) == bool(yv)
                res = pm_call(LC.pm_inputs(M, K, Co, ep), out=out)
                assert res.data_ptr() == out.data_ptr()
                e = LC.expect(c, 0, M, K, Co, y_aligned=bool(yv))
                assert e[5] == yv
                last(e, what)
                same(res, "pm_%d_%d_%d_%s" % (M, K, Co, ep), what)
                host = big.cpu().numpy()
                assert (host[:lead] == LC.SENTINEL).all() and (host[lead + n:] == LC.SENTINEL).all(), "%s: guard elements were written" % what

    # ---- operands off the 16-byte grid: x and w as contiguous views 1 float into their buffers -> 4-byte loads, no DMA, same bits
    M, K, Co = LC.OFFGRID_CASE
    for ep in LC.PM_EPILOGUES:
        what = "operands off the 16-byte grid M=%d K=%d Co=%d epilogue %s" % (M, K, Co, ep)
        d = LC.pm_inputs(M, K, Co, ep)
        xb, wb = torch.zeros(M * K + 5, device="cuda"), torch.zeros(Co * K + 5, device="cuda")
        xv, wv = xb[1:1 + M * K].view(M, K), wb[1:1 + Co * K].view(Co, K)
        xv.copy_(dev(d["x"])), wv.copy_(dev(d["w"]))
        assert xv.is_contiguous() and wv.is_contiguous() and xv.data_ptr() % 16 == 4 and wv.data_ptr() % 16 == 4
        got = pm_call(d, x=xv, w=wv)
        e = LC.expect(c, 0, M, K, Co, aligned=False)
        assert e[2] == 0 and e[4] == 0
        last(e, what)
        same(got, "pm_%d_%d_%d_%s" % (M, K, Co, ep), what)

    torch.cuda.synchronize()
    assert used == set(refs.files), sorted(set(refs.files) - used)
    assert seen == LC.expected_triples(c), (sorted(seen), sorted(LC.expected_triples(c)))
    print("TRIPLES %r" % sorted(seen))
    print("DIGEST %s" % digest.hexdigest())
    print("ALL COMPARED cfg=%d references=%d" % (c, len(used)))
