"""Write esmstereo_amd/colormaps.json: the 256-entry `jet` and `magma` tables of matplotlib, as uint8 RGB.
The file is text: per table 256 entries of six hex digits, "rrggbb", sixteen to a line.

    python scripts/make_colormaps.py

Each table is rint(cmap(arange(256))[:, :3] * 255) of matplotlib's registered colormap (generated with matplotlib
3.10.8; the tables are data, the package imports neither matplotlib nor cv2 at run time).  These are matplotlib's
tables: OpenCV's COLORMAP_JET is its own table and differs from matplotlib's jet, and no parity with OpenCV is
claimed for either, so a caller who wants cv2's bytes passes
cv2.applyColorMap(np.arange(256, dtype=np.uint8), code)[:, 0] as the table instead.
Run once where matplotlib is installed; the result is committed."""
import json
import os

import numpy as np

NAMES = ("jet", "magma")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esmstereo_amd", "colormaps.json")


def table(name: str) -> np.ndarray:
    import matplotlib

    rgba = matplotlib.colormaps[name](np.arange(256))
    return np.rint(rgba[:, :3] * 255).astype(np.uint8)


def main() -> None:
    import matplotlib

    tabs = {n: table(n) for n in NAMES}
    doc = {"matplotlib_version": matplotlib.__version__, "format": "256 x rrggbb, sixteen entries per string"}
    for n, t in tabs.items():
        hexes = ["%02x%02x%02x" % tuple(int(c) for c in e) for e in t]
        doc[n] = [" ".join(hexes[i:i + 16]) for i in range(0, 256, 16)]
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for n, t in tabs.items():
        print(n, t.shape, t.dtype, t[0], t[128], t[255])
    print("wrote", OUT)


if __name__ == "__main__":
    main()
