'use strict';
// node group_smoke.js <out_dir> <device ids as JSON, e.g. [0,0,0,0]>: one image on a device group vs one device.
// Writes group.json: for 1 frame and for 12 frames at 8 per launch, whether readAccum() of the group equals the
// { device: 0 } renderer's bit for bit.
const fs = require('fs');
const path = require('path');
const { Volxel3DDicomRenderer, native } = require('./index');
const out = process.argv[2];
const devices = JSON.parse(process.argv[3]);
const n = 32;
const vox = new Uint16Array(n * n * n);
for (let z = 0; z < n; ++z) for (let y = 0; y < n; ++y) for (let x = 0; x < n; ++x) {
  const c = (n - 1) / 2, r = 28 * n / 64;
  const d = Math.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2);
  vox[(z * n + y) * n + x] = Math.round(4095 * Math.max(0, 1 - d / r));
}
const grid = native.buildBrickGrid(vox, [n, n, n], [1, 1, 1], 0, 2);
function make(opts) {
  const r = new Volxel3DDicomRenderer(Object.assign({ width: 96, height: 64 }, opts));
  r.setupFromGrid(grid);
  r.settings.renderMode = 'dvr'; r.settings.bounces = 1;
  return r;
}
function same(a, b) {
  if (a.length !== b.length) return false;
  const ua = new Uint32Array(a.buffer, a.byteOffset, a.length), ub = new Uint32Array(b.buffer, b.byteOffset, b.length);
  for (let i = 0; i < ua.length; ++i) if (ua[i] !== ub[i]) return false;
  return true;
}
const one = make({ device: 0 }), group = make({ devices });
const res = { devices: group.devices };
one.render(1); group.render(1);
res.oneFrame = same(one.readAccum(), group.readAccum());
one.restartRendering(); group.restartRendering();
one.render(12, 8); group.render(12, 8);
const a = one.readAccum(), b = group.readAccum();
res.twelveFrames = same(a, b);
res.nonzero = a.some(v => v !== 0 && v !== 1);
res.frameIndex = group.frameIndex;
res.samples = [one.counters().samples, group.counters().samples];
let both = '';
try { new Volxel3DDicomRenderer({ device: 0, devices }); } catch (e) { both = e.message; }
res.bothRefused = both;
one.dispose(); group.dispose();
fs.writeFileSync(path.join(out, 'group.json'), JSON.stringify(res));
