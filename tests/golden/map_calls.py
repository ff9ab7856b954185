"""What a ResultLogger.draw_trajectory hands to matplotlib, as data: every Axes.plot / Axes.scatter call in order, with its
coordinates as float64 lists and its style arguments normalised to plain values.  Shared by make_golden_map.py (which records
the reference's calls into result_map.npz) and tests/test_globalmap_fixture.py (which records ours)."""
import contextlib

import numpy as np

STYLE = ("color", "c", "marker", "markersize", "markeredgewidth", "markeredgecolor", "linestyle", "alpha", "zorder", "s")


def _plain(v):
    if isinstance(v, str):
        return v
    a = np.asarray(v, dtype=np.float64).ravel()
    return [float(x) for x in a] if a.size > 1 else float(a[0])


def _coords(v):
    if isinstance(v, (list, tuple)):
        return [float(np.asarray(x, dtype=np.float64)) for x in v]
    return np.asarray(v, dtype=np.float64).ravel().tolist()


@contextlib.contextmanager
def recording():
    """-> list that receives {fn, x, y, style} per Axes.plot / Axes.scatter call made inside the block (Agg backend)"""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib.axes import Axes
    calls = []
    orig = Axes.plot, Axes.scatter

    def plot(self, x, y, *a, **k):
        calls.append(dict(fn="plot", x=_coords(x), y=_coords(y), style={n: _plain(k[n]) for n in STYLE if n in k}))
        return orig[0](self, x, y, *a, **k)

    def scatter(self, x, y, *a, **k):
        calls.append(dict(fn="scatter", x=_coords(x), y=_coords(y), style={n: _plain(k[n]) for n in STYLE if n in k}))
        return orig[1](self, x, y, *a, **k)

    Axes.plot, Axes.scatter = plot, scatter
    try:
        yield calls
    finally:
        Axes.plot, Axes.scatter = orig


def is_map_layer(call) -> bool:
    """the two voxel-map scatters (zorder 4 / 5) -- compared as point sets, not element by element"""
    return call["fn"] == "scatter" and call["style"].get("zorder") in (4.0, 5.0)
