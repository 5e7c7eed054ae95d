#!/usr/bin/env python3
"""Inference with precise (vertex-to-point) maps beside the vertex maps (ops.precise_map; not in the reference).

This is the inference driver itself — test_driver.main, called with every argument given here, so its options, defaults and
`--help` are the ones in force and its T/T_<a>_<b>.txt and feature/usefeature_<a>.mat are written by its own code — with one
addition: at the point where it writes a pair's results, the precise maps of both directions are written beside them from the
same features,

    <out>/P/P_<a>_<b>.txt    one line per source point of <a>: `face w0 w1 w2` — the 1-based triangle of <b> and the three
                             barycentric weights ('%.9g') of the closest point of <b>'s mesh in feature space.

The triangles come from the data root's meshes (--data-root) or from optional faces1 / faces2 (F,3) arrays of a --pairs file.
Shapes without triangles (synthetic pairs, point-cloud sets, a --pairs file without the arrays) are an error before the backbone
runs.

  python dv-matcher_amd/precise_driver.py --pairs pair.npz --out result/demo [--ckpt ep_val_best.pth]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_driver  # noqa: E402
from dvm import ops  # noqa: E402
from eval_geodesic import map_dirichlet_energy  # noqa: E402


def load_faces(args):
    """{shape name: faces (F,3) int32} for every shape of the pairs the inference driver will run; raises ValueError where a shape
    has no triangles.  args: data_root, data_name, pairs as the inference driver reads them."""
    def need(faces, name, where):
        if faces is None or not len(faces):
            raise ValueError("precise maps need the triangles of every shape, and %s has none (%s)" % (name, where))
        return np.ascontiguousarray(np.asarray(faces).reshape(-1, 3)).astype(np.int32)

    if args.data_root:
        from models.dataset import testDataset
        data = testDataset(args.data_root, name=args.data_name, train=False)   # (leaves the cache the driver's own load then reads)
        tris = data.faces_list
        where = "the set %s holds bare point clouds" % args.data_name
        used = sorted({i for pair in data.combinations for i in pair})
        return {data.used_shapes[i]: need(None if tris is None else tris[i], data.used_shapes[i], where) for i in used}
    if args.pairs:
        out = {}
        for path in args.pairs:
            d = np.load(path, allow_pickle=False)
            where = "%s carries no faces1 / faces2 arrays" % path
            for k in ("1", "2"):
                name = str(d["name" + k])
                out[name] = need(d["faces" + k] if "faces" + k in d.files else None, name, where)
        return out
    raise ValueError("precise maps need the triangles of every shape, and synthetic pairs have none: pass --data-root or --pairs")


def load_verts(args):
    """{shape name: verts (N,3) float32} of the shapes load_faces names, from the same source (for the maps' Dirichlet energy)."""
    if args.data_root:
        from models.dataset import testDataset
        data = testDataset(args.data_root, name=args.data_name, train=False)
        used = sorted({i for pair in data.combinations for i in pair})
        return {data.used_shapes[i]: np.asarray(data.verts_list[i], dtype=np.float32) for i in used}
    out = {}
    for path in args.pairs:
        d = np.load(path, allow_pickle=False)
        for k in ("1", "2"):
            out[str(d["name" + k])] = np.asarray(d["verts" + k], dtype=np.float32)
    return out


def write_precise(save_path, name_src, name_tgt, face, bary):
    pdir = os.path.join(save_path, "P")
    os.makedirs(pdir, exist_ok=True)
    with open(os.path.join(pdir, "P_%s_%s.txt" % (name_src, name_tgt)), "w") as f:
        for fc, w in zip(face.tolist(), bary.tolist()):
            f.write("%d %.9g %.9g %.9g\n" % (fc + 1, w[0], w[1], w[2]))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    # the three arguments that say where the shapes come from are read here as well, under the inference driver's names; everything
    # else (and -h) is its parser's alone
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--pairs", nargs="*", default=None)
    ap.add_argument("--data-root", default=None)
    ap.add_argument("--data-name", default="scape_r")
    args, _ = ap.parse_known_args(argv)
    if not ({"-h", "--help"} & set(argv)):
        tris = load_faces(args)                    # (before the backbone runs: a shape without triangles is an argument error)
        xyz = load_verts(args)
    written = test_driver.write_results

    def write_with_precise(save_path, name1, name2, T12, T21, feat1, feat2):
        """The inference driver's write_results, then the two P files from the features it was handed."""
        written(save_path, name1, name2, T12, T21, feat1, feat2)
        dev = torch.device("cuda", torch.cuda.current_device())
        f = {name1: torch.from_numpy(np.ascontiguousarray(feat1, dtype=np.float32)).to(dev)[None],
             name2: torch.from_numpy(np.ascontiguousarray(feat2, dtype=np.float32)).to(dev)[None]}
        for src, tgt, T in ((name1, name2, T12), (name2, name1, T21)):
            face, bary, _, _ = ops.precise_map(f[src], f[tgt], torch.from_numpy(tris[tgt]).to(dev), want_dist=False)
            face, bary = face[0].cpu().numpy(), bary[0].cpu().numpy()
            write_precise(save_path, src, tgt, face, bary)
            # the smoothness of both maps (eval_geodesic.map_dirichlet_energy: 1 = local lengths kept); printed, no file
            print(json.dumps({"pair": [src, tgt],
                              "dirichlet_vertex": map_dirichlet_energy(xyz[src], tris[src], xyz[tgt], T=np.asarray(T).reshape(-1) - 1),   # (the T files are 1-based)
                              "dirichlet_precise": map_dirichlet_energy(xyz[src], tris[src], xyz[tgt], face=face, bary=bary, faces_tgt=tris[tgt])}))

    test_driver.write_results = write_with_precise
    try:
        test_driver.main(argv)
    finally:
        test_driver.write_results = written


if __name__ == "__main__":
    main()
