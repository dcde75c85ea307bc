"""Helpers shared by the parity tests: loading tests/golden/*.npz (vectors produced by the real
reference, see oracle/gen_golden.py) and turning them into oracle / product inputs."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def names(prefix=None):
    out = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "*.npz")))
    if prefix is not None:
        pre = (prefix,) if isinstance(prefix, str) else tuple(prefix)
        out = [n for n in out if n.startswith(pre)]
    return out


class Fixture(dict):
    """A fixture's arrays with the `.files` of np.load's NpzFile (for fixtures that have stored pieces)."""

    @property
    def files(self):
        return list(self)


def load(name, golden=GOLDEN):
    """A fixture (of tests/golden/, or of another directory of the same layout).  A row too large for one committed
    file sits beside it as consecutive pieces rows/<name>.<key>.<k>.npz (oracle/gen_golden.py), joined here whole."""
    z = np.load(os.path.join(golden, name + ".npz"))
    pieces = sorted(glob.glob(os.path.join(golden, "rows", glob.escape(name) + ".*.*.npz")))
    if not pieces:
        return z
    g = Fixture((k, z[k]) for k in z.files)
    rows = {}
    for f in pieces:
        key, k = os.path.basename(f)[len(name) + 1:-4].rsplit(".", 1)
        rows.setdefault(key, []).append((int(k), np.load(f)["rows"]))
    for key, parts in rows.items():
        g[key] = np.concatenate([a for _, a in sorted(parts, key=lambda p: p[0])])
    return g


def node_dict(g):
    return dict(is_reverse=g["node_is_reverse_node"], turn=g["node_turn"], stop=g["node_stop"],
                wait_time=g["node_wait_time"], max_velocity=g["node_max_velocity"],
                max_acceleration=g["node_max_acceleration"], tangent=g["node_tangent"],
                magnitudes=np.nan_to_num(g["node_magnitudes"]))


def action_dict(g):
    if "ap_t" not in g.files:
        return None
    return dict(t=g["ap_t"], stop=g["ap_stop"], wait_time=g["ap_wait_time"],
                max_velocity=g["ap_max_velocity"], max_acceleration=g["ap_max_acceleration"])


def ref_segments(g):
    ns = int(g["n_splines"])
    seg = np.concatenate([g[f"spline{i}_segments"] for i in range(ns)])
    sl = np.concatenate([g[f"spline{i}_segment_lengths"] for i in range(ns)])
    pl = np.array([float(g[f"spline{i}_param_last"]) for i in range(ns)])
    return seg, sl, pl
