"""Record what the reference's plotLines (wisetools.py:527-662) draws for the cases of tests/plot_cases.py.

The routine stops on today's matplotlib at a removed tick attribute, so the names `plt` and `matplotlib` of the loaded
reference module (tools/ref_loader.py) are replaced by unittest.mock.MagicMock objects: the routine then runs to its
end and every axhline, axvline, text, plot, xlim, ylabel and patches.Rectangle call is on record with its arguments.
Only plain arrays and strings of those records go to tests/golden/plot_primitives.npz; no reference text does.

    python tools/make_plot_golden.py
"""
import os
import sys
import tempfile
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "plot_primitives.npz")
HATCH = {None: 0, '//': 1, '\\': 2}


def _rgb(colour):
    return (0.0, 0.0, 0.0) if colour == 'black' else tuple(float(v) for v in colour)


def record(case, ref_wt, cyto_path):
    plt, mpl = mock.MagicMock(), mock.MagicMock()
    root = mock.MagicMock()
    root.attach_mock(plt, 'plt')
    root.attach_mock(mpl, 'matplotlib')
    with mock.patch.object(ref_wt, 'plt', plt), mock.patch.object(ref_wt, 'matplotlib', mpl):
        ref_wt.plotLines(case['zscores'], case['calls'], np.array(case['threshold']), sampleName=case['sample'],
                         binsize=np.array(case['binsize']), cytoFile=cyto_path if case['cyto'] else None,
                         chromosomes=case['chromosomes'], columns=case['columns'], size=list(case['size']),
                         minEffect=case['mineffect'])
    panel = -1
    hline, vline, rect, text_at, text_s, text_va, xlim, ylabel, plot_len, plot_y, grid = [], [], [], [], [], [], [], [], [], [], []
    title, legend, legend_rgb = '', [], []
    for name, args, kw in root.mock_calls:
        if name == 'plt.subplot':
            panel = int(args[2]) - 1
            grid.append((panel, int(args[0]), int(args[1])))
        elif name == 'plt.axhline':
            hline.append((panel, float(kw['y'])) + _rgb(kw['color']))
        elif name == 'plt.axvline':
            vline.append((panel, float(kw['x'])) + _rgb(kw['color']))
        elif name == 'matplotlib.patches.Rectangle':
            (x, y), w, h = args
            rect.append((panel, float(x), float(y), float(w), float(h)) + _rgb(kw.get('color', kw.get('facecolor'))) +
                        (float(kw['alpha']), HATCH[kw.get('hatch')]))
        elif name == 'plt.text':
            text_at.append((panel, float(args[0]), float(args[1])))
            text_s.append(str(args[2]))
            text_va.append(str(kw['verticalalignment']))
        elif name == 'plt.xlim':
            xlim.append((panel, float(args[0]), float(args[1])))
        elif name == 'plt.ylabel':
            ylabel.append((panel, int(args[0])))
        elif name == 'plt.plot':
            y = np.asarray(args[0], dtype=np.float64)
            plot_len.append((panel, len(y)) + _rgb(kw['color']))
            plot_y.append(y)
        elif name == 'plt.figure().text':
            title = str(args[2])
        elif name == 'plt.Rectangle':
            legend_rgb.append(_rgb(kw['fc']))
        elif name == 'plt.figure().legend':
            legend = [str(v) for v in args[1]]
    f8 = np.float64
    return dict(hline=np.array(hline, f8).reshape(-1, 5), vline=np.array(vline, f8).reshape(-1, 5),
                rect=np.array(rect, f8).reshape(-1, 10), text_at=np.array(text_at, f8).reshape(-1, 3),
                text_s=np.array(text_s, dtype='U32'), text_va=np.array(text_va, dtype='U8'), xlim=np.array(xlim, f8).reshape(-1, 3),
                ylabel=np.array(ylabel, np.int64).reshape(-1, 2), plot_len=np.array(plot_len, f8).reshape(-1, 5),
                plot_y=np.concatenate(plot_y) if plot_y else np.zeros(0), grid=np.array(grid, np.int64).reshape(-1, 3),
                title=np.array(title), legend=np.array(legend, dtype='U32'), legend_rgb=np.array(legend_rgb, f8).reshape(-1, 3))


def main():
    import plot_cases
    import ref_loader
    ref_wt = ref_loader.load()[0]
    stored = {}
    with tempfile.TemporaryDirectory() as tmp:
        cyto_path = os.path.join(tmp, "cytoBand.txt")
        with open(cyto_path, "w") as f:
            f.write(plot_cases.CYTO_TEXT)
        names = []
        for case in plot_cases.cases():
            names.append(case['name'])
            for key, value in record(case, ref_wt, cyto_path).items():
                stored["%s__%s" % (case['name'], key)] = value
    stored["cases"] = np.array(names, dtype='U32')
    np.savez_compressed(OUT, **stored)
    print(OUT, os.path.getsize(OUT), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
