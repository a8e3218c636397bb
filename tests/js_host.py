"""The node harness of the test_js_host_* tests: the grid written to files, the script prelude that loads it into a
Volxel3DDicomRenderer as the Python tests' renderer() does, and the child process that runs prelude + body."""
import json
import subprocess

import numpy as np

from tests.common import NAPI
from volxel_amd.settings import BENCHMARK_SETTINGS


def dump_grid(tmp_path, g):
    """grid.json, ind.bin / range.bin / atlas.bin / mipN.bin and settings.json (the benchmark settings) under tmp_path"""
    (tmp_path / "grid.json").write_text(json.dumps({
        "indirectionSize": list(map(int, g.indirection_size)), "rangeSize": list(map(int, g.range_size)),
        "atlasSize": list(map(int, g.atlas_size)), "indexExtent": list(map(int, g.index_extent)),
        "minMaj": list(map(float, g.min_maj)), "transform": list(map(float, g.transform)),
        "mips": [list(map(int, sz)) for _, sz in g.range_mipmaps]}))
    np.asarray(g.indirection, dtype=np.uint32).tofile(tmp_path / "ind.bin")
    np.asarray(g.range, dtype=np.uint16).tofile(tmp_path / "range.bin")
    np.asarray(g.atlas, dtype=np.uint8).tofile(tmp_path / "atlas.bin")
    for i, (mm, _) in enumerate(g.range_mipmaps):
        np.asarray(mm, dtype=np.uint16).tofile(tmp_path / f"mip{i}.bin")
    (tmp_path / "settings.json").write_text(json.dumps(BENCHMARK_SETTINGS))


# in scope for the body: fs, path, napi, dir, v (the module), rd, save, g, grid and r, a renderer of the size run_node passes
PRELUDE = r"""
const fs = require('fs'), path = require('path');
const [napi, dir, width, height] = process.argv.slice(2);
const v = require(napi);
const rd = (f, T) => { const b = fs.readFileSync(path.join(dir, f)); return new T(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const save = (f, m) => fs.writeFileSync(path.join(dir, f), Buffer.from(m.buffer, m.byteOffset, m.byteLength));
const g = JSON.parse(fs.readFileSync(path.join(dir, 'grid.json')));
const grid = { type: 'return_dicom', indirectionSize: g.indirectionSize, rangeSize: g.rangeSize, atlasSize: g.atlasSize,
  indexExtent: g.indexExtent, minMaj: g.minMaj, transform: new Float32Array(g.transform),
  indirection: rd('ind.bin', Uint32Array), range: rd('range.bin', Uint16Array), atlas: rd('atlas.bin', Uint8Array),
  rangeMipmaps: g.mips.map((s, i) => ({ mipmap: rd(`mip${i}.bin`, Uint16Array), stride: s })) };
const r = new v.Volxel3DDicomRenderer({ width: Number(width), height: Number(height) });
r.setupFromGrid(grid);
r.restoreSettings(JSON.parse(fs.readFileSync(path.join(dir, 'settings.json'))));
r.settings.renderMode = 'dvr';
"""


def run_node(tmp_path, body, timeout=300, size=(64, 48)):
    """builds the napi module, runs PRELUDE + body in a fresh node process on the files of dump_grid, and returns the JSON of
    the last line it printed; a non-zero exit fails with the tail of stderr"""
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = tmp_path / "s.js"
    script.write_text(PRELUDE + body)
    out = subprocess.run(["node", str(script), NAPI, str(tmp_path), str(size[0]), str(size[1])], capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])
