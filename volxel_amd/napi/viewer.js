'use strict';
/**
 * Headless JavaScript host over the N-API shim: keeps the public surface of the reference's
 * render core (class Volxel3DDicomRenderer, volxel-3d-viewer/src/viewer.ts) for the calls on
 * the hot path -- setupFromGrid (viewer.ts:1080-1145), changeTransferFunc (:1147-1153),
 * restartRendering (:1155-1181), bindUniforms (:1295-1357), render (:1183-1293), renderMode
 * (:1442-1452), restoreSettings (:704-713) -- and of utils/data.ts (generateTransferFunction).
 * The reference is TypeScript + math.gl in a browser; the build image has Node 12 without tsc,
 * so this is plain ES2019 with the typings in index.d.ts.  Everything that touches pixels goes
 * through libvolxel_hip.so; there is no JavaScript fallback.
 */
const fs = require('fs');
const path = require('path');
const native = require('./volxel_napi.node');
const nativeDistance = require('./volxel_napi_distance.node');   // the addon of the distance calls, on native's handles
const nativeSegments = require('./volxel_napi_segments.node');   // the addon of the segment store, on native's handles
const nativeHistogram = require('./volxel_napi_histogram.node'); // the addon of the histograms, on native's handles

const RenderMode = Object.freeze({ default: 0, no_dda: 1, raymarch: 2, dvr: 3, dvr_phong: 4, mip: 5, minip: 6 });
const LOW_RES_DURATION = 5; // viewer.ts:132

// ---- VxParams / VxSliceParams field tables, parsed from the C header (single source of truth) --------------
function parseParamsLayout(name = 'VxParams', size = native.sizeofParams()) {
  const text = fs.readFileSync(path.join(__dirname, '..', '..', 'include', 'volxel_hip.h'), 'utf8')
    .replace(/\/\*[\s\S]*?\*\//g, '');
  const body = new RegExp(`typedef\\s+struct\\s+${name}\\s*\\{([\\s\\S]*?)\\}\\s*${name}\\s*;`).exec(text)[1];
  const fields = {};
  let off = 0;
  for (const decl of body.split(';')) {
    const m = /^\s*(\w+)\s+([\s\S]+)$/.exec(decl);
    if (!m) continue;
    for (const item of m[2].split(',')) {
      const a = /^\s*(\w+)\s*(?:\[(\d+)\])?\s*$/.exec(item);
      const n = a[2] ? parseInt(a[2], 10) : 1;
      fields[a[1]] = { type: m[1], offset: off, count: n };
      off += 4 * n;
    }
  }
  if (off !== size) throw new Error(`${name} layout mismatch between header and library`);
  return { fields, size: off };
}
const LAYOUT = parseParamsLayout();
const SLICE_LAYOUT = parseParamsLayout('VxSliceParams', native.sizeofSliceParams());
const ISO_LAYOUT = parseParamsLayout('VxIsoParams', native.sizeofIsoParams());
const SEGMENT_LAYOUT = parseParamsLayout('VxSegmentParams', native.sizeofSegmentParams());
const MESH_LAYOUT = parseParamsLayout('VxMeshParams', native.sizeofMeshParams());
const HISTOGRAM_LAYOUT = parseParamsLayout('VxHistogramParams', nativeHistogram.sizeofHistogramParams());
const HIST_MAX_BINS = 4096;                               // VX_HIST_MAX_BINS
const RADIX_PASSES = [[0, 11], [11, 11], [22, 10]];       // [prefix_bits, key_bits] of the three passes of the radix select
const MESH_SPACES = ['voxel', 'grid', 'world'];
const SEGMENT_VIEWS = ['off', 'only', 'hide'];   // VX_SEGVIEW_OFF, _ONLY, _HIDE
const SEGMENT_EDIT_OPS = ['dilate', 'erode', 'open', 'close', 'fill_holes'];   // VxSegmentEditOp, in order
const MARGIN_OPS = ['grow', 'shrink', 'open', 'close'];   // VxMarginOp, in order
const DISTANCE_SIDES = ['outside', 'inside'];             // VxDistanceSide, in order
const COMBINE_OPS = ['union', 'intersect', 'subtract', 'xor', 'invert'];   // VxCombineOp, in order
const SEGMENT_SLOTS = 32;                                 // VX_SEGMENT_SLOTS
const SliceReduce = Object.freeze({ mean: 0, max: 1, min: 2 });         // enum VxSliceReduce
const SliceDisplay = Object.freeze({ grey: 1, tf: 2 });                  // enum VxSliceDisplay (null: VX_SLICE_NONE)

class ParamsBlock {
  constructor(layout = LAYOUT) { this.layout = layout; this.buffer = new ArrayBuffer(layout.size); this.view = new DataView(this.buffer); }
  set(name, value) {
    const f = this.layout.fields[name];
    if (!f) throw new Error(`unknown uniform ${name}`);
    const vals = (typeof value === 'number') ? [value] : Array.from(value);
    if (vals.length !== f.count) throw new Error(`uniform ${name} expects ${f.count} values`);
    vals.forEach((v, i) => {
      const o = f.offset + 4 * i;
      if (f.type === 'float') this.view.setFloat32(o, v, true);
      else if (f.type === 'uint32_t') this.view.setUint32(o, v, true);
      else this.view.setInt32(o, v, true);
    });
  }
}

// ---- column-major 4x4 helpers in doubles (gl-matrix conventions used through math.gl) ------
const M = {
  identity: () => [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1],
  mul(a, b) { // a * b
    const o = new Array(16).fill(0);
    for (let c = 0; c < 4; ++c) for (let r = 0; r < 4; ++r)
      for (let k = 0; k < 4; ++k) o[4 * c + r] += a[4 * k + r] * b[4 * c + k];
    return o;
  },
  scale: (s) => [s[0], 0, 0, 0, 0, s[1], 0, 0, 0, 0, s[2], 0, 0, 0, 0, 1],
  translate: (t) => [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, t[0], t[1], t[2], 1],
  apply(m, v) { return [0, 1, 2, 3].map(r => m[r] * v[0] + m[4 + r] * v[1] + m[8 + r] * v[2] + m[12 + r] * v[3]); },
  lookAt(eye, center, up) { // scene.ts:58-64
    let z = [eye[0] - center[0], eye[1] - center[1], eye[2] - center[2]];
    if (z.every(c => Math.abs(c) < 1e-6)) return M.identity();
    const n = (v) => { const l = Math.hypot(v[0], v[1], v[2]); return l ? v.map(c => c / l) : [0, 0, 0]; };
    const cross = (a, b) => [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]];
    const dot = (a, b) => a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    z = n(z);
    const x = n(cross(up, z));
    const y = n(cross(z, x));
    return [x[0], y[0], z[0], 0, x[1], y[1], z[1], 0, x[2], y[2], z[2], 0, -dot(x, eye), -dot(y, eye), -dot(z, eye), 1];
  },
  perspective(fovy, aspect, near, far) { // scene.ts:65-72
    const f = 1 / Math.tan(fovy / 2), nf = 1 / (near - far);
    return [f / aspect, 0, 0, 0, 0, f, 0, 0, 0, 0, (far + near) * nf, -1, 0, 0, 2 * far * near * nf, 0];
  },
  ortho(left, right, bottom, top, near, far) { // gl-matrix mat4.ortho; [build]: the reference camera is perspective only
    const lr = 1 / (left - right), bt = 1 / (bottom - top), nf = 1 / (near - far);
    return [-2 * lr, 0, 0, 0, 0, -2 * bt, 0, 0, 0, 0, 2 * nf, 0, (left + right) * lr, (top + bottom) * bt, (far + near) * nf, 1];
  },
  invert(m) { // Gauss-Jordan with partial pivoting on the 4x4
    const a = [0, 1, 2, 3].map(r => [m[r], m[4 + r], m[8 + r], m[12 + r], +(r === 0), +(r === 1), +(r === 2), +(r === 3)]);
    for (let c = 0; c < 4; ++c) {
      let p = c;
      for (let r = c + 1; r < 4; ++r) if (Math.abs(a[r][c]) > Math.abs(a[p][c])) p = r;
      if (a[p][c] === 0) throw new Error('singular matrix');
      [a[c], a[p]] = [a[p], a[c]];
      const d = a[c][c];
      for (let k = 0; k < 8; ++k) a[c][k] /= d;
      for (let r = 0; r < 4; ++r) if (r !== c) { const f = a[r][c]; for (let k = 0; k < 8; ++k) a[r][k] -= f * a[c][k]; }
    }
    const o = new Array(16);
    for (let r = 0; r < 4; ++r) for (let c = 0; c < 4; ++c) o[4 * c + r] = a[r][4 + c];
    return o;
  },
  f32: (m) => Array.from(new Float32Array(m)),
};

// ---- utils/data.ts:21-60 ---------------------------------------------------------------
function generateTransferFunction(colors, generatedSteps = 128) {
  if (colors.length < 1) throw new Error('At least one color stop required');
  const stops = colors.slice().sort((a, b) => a.stop - b.stop);
  if (stops.some(s => s.stop < 0 || s.stop > 1)) throw new Error('ColorStop outside stop range');
  const out = [];
  let cur = -1;
  for (let i = 0; i < generatedSteps; ++i) {
    const pos = i / generatedSteps;
    if (cur < 0) {
      if (stops[0].stop >= pos) { cur = 0; out.push(stops[0].color); } else out.push([0, 0, 0, 0]);
      continue;
    }
    const next = stops[cur + 1];
    if (!next) { out.push(stops[cur].color); continue; }
    const w = (pos - stops[cur].stop) / (next.stop - stops[cur].stop);
    if (w >= 1) { out.push(next.color); cur++; continue; }
    out.push(stops[cur].color.map((v, k) => (1 - w) * v + w * next.color[k]));
  }
  return { data: new Float32Array(out.flat()), length: generatedSteps };
}

// math.gl Quaternion / Vector3 pieces used by the orbit camera (gl-matrix quat.setAxisAngle, quat.multiply, vec3.transformQuat)
const Q = {
  axis: (a, rad) => { const s = Math.sin(rad * 0.5); return [a[0] * s, a[1] * s, a[2] * s, Math.cos(rad * 0.5)]; },
  mul: (a, b) => [a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1], a[1] * b[3] + a[3] * b[1] + a[2] * b[0] - a[0] * b[2],
    a[2] * b[3] + a[3] * b[2] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]],
  rot: (v, q) => {
    const cross = (a, b) => [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]];
    const uv = cross(q, v), uuv = cross(q, uv);
    return [0, 1, 2].map(i => v[i] + 2 * q[3] * uv[i] + 2 * uuv[i]);
  },
};
const V = {
  sub: (a, b) => a.map((x, i) => x - b[i]), add: (a, b) => a.map((x, i) => x + b[i]), scale: (a, s) => a.map(x => x * s),
  len: a => Math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), norm: a => V.scale(a, 1 / V.len(a)),
  cross: (a, b) => [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]],
};

class Camera { // representation/scene.ts
  // orthoHalfHeight ([build], BASELINE config 1): null = the reference's perspective camera
  constructor(distance = 1) { this.view = [0, 0, 0]; this.pos = [0, 0, -distance]; this.orthoHalfHeight = null; this.yaw = 0; this.pitch = 0; }
  rotateAroundView(by) { // scene.ts:15-33
    this.yaw += -by[0]; this.pitch += by[1];
    const maxPitch = Math.PI / 2 - 0.01;
    this.pitch = Math.min(Math.max(this.pitch, -maxPitch), maxPitch);
    const qYaw = Q.axis([0, 1, 0], this.yaw);
    const right = V.norm(Q.rot([1, 0, 0], qYaw));
    const orientation = Q.mul(Q.axis(right, this.pitch), qYaw);
    this.pos = V.add(V.scale(Q.rot([0, 0, -1], orientation), V.len(V.sub(this.pos, this.view))), this.view);
  }
  zoom(by) { // scene.ts:35-40
    const dir = V.sub(this.pos, this.view), n = V.len(dir);
    if (n * by <= 0.1 || n * by >= 10) return false;
    this.pos = V.add(V.scale(dir, by), this.view);
    return true;
  }
  translateOnPlane(by) { // scene.ts:42-47
    const dir = V.sub(this.pos, this.view), right = V.norm(V.cross(dir, [0, 1, 0])), localUp = V.norm(V.cross(dir, right));
    this.translate(V.add(V.scale(right, by[0] * 5), V.scale(localUp, -by[1] * 5)));
  }
  translate(by) { this.pos = V.add(this.pos, by); this.view = V.add(this.view, by); } // scene.ts:49-52
  viewMatrix() { return M.lookAt(this.pos, this.view, [0, 1, 0]); }
  projMatrix(aspect, fov = Math.PI / 3) {
    if (this.orthoHalfHeight !== null) {
      const h = this.orthoHalfHeight;
      return M.ortho(-h * aspect, h * aspect, -h, h, 0.1, 1000);
    }
    return M.perspective(fov, aspect, 0.1, 1000);
  }
}

/** representation/environment.ts: base map = width x height RGBA floats, row 0 = TOP */
class Environment {
  constructor(floats, width, height, strength = 1) {
    if (floats.length !== width * height * 4) throw new Error('Environment: floats must hold width*height RGBA texels');
    this.floats = floats; this.width = width; this.height = height; this.strength = strength;
  }
  static default() { // environment.ts:102-130, 8x6 checkerboard with a bright upper third
    const width = 8, height = 6, d = new Float32Array(width * height * 4);
    for (let y = 0; y < height; ++y) {
      const top = y < Math.floor(height / 3);
      for (let x = 0; x < width; ++x) {
        const light = ((x + y) & 1) === 0, val = top ? (light ? 3 : 0.9) : (light ? 0.1 : 0.0), i = (y * width + x) * 4;
        d[i] = d[i + 1] = d[i + 2] = val; d[i + 3] = 1;
      }
    }
    return new Environment(d, width, height);
  }
}

// ---- container I/O behind the load methods (not on the hot path; what Node's own zlib / fs can decode) ------------
/** zip.rs:36-115: files in archive order, at most one directory entry, every later file directly inside it */
function readZipSlices(buf) {
  const zlib = require('zlib');
  const fail = (kind, msg) => { throw new Error(`${kind}: ${msg === undefined ? 'No Message Specified' : msg}`); };
  let eocd = -1;
  for (let i = buf.length - 22; i >= Math.max(0, buf.length - 65557); --i) if (buf.readUInt32LE(i) === 0x06054b50) { eocd = i; break; }
  if (eocd < 0) fail('ExtractFailed', 'invalid Zip archive: Could not find central directory end');
  const total = buf.readUInt16LE(eocd + 10);
  let p = buf.readUInt32LE(eocd + 16);
  if (total < 1) fail('NoFiles');
  let directory = null;
  const out = [];
  for (let k = 0; k < total; ++k) {
    if (buf.readUInt32LE(p) !== 0x02014b50) fail('ExtractFailed', 'invalid central directory entry');
    const method = buf.readUInt16LE(p + 10), csize = buf.readUInt32LE(p + 20), nlen = buf.readUInt16LE(p + 28),
      xlen = buf.readUInt16LE(p + 30), clen = buf.readUInt16LE(p + 32), lho = buf.readUInt32LE(p + 42);
    const name = buf.toString('utf8', p + 46, p + 46 + nlen);
    p += 46 + nlen + xlen + clen;
    const norm = require('path').posix.normalize(name);
    if (name.startsWith('/') || norm.startsWith('..')) fail('ExtractFailed', 'No enclosed name was able to be found');
    if (name.endsWith('/')) {
      if (directory !== null) fail('MoreThanOneFolder');
      directory = norm.replace(/\/$/, '');
      continue;
    }
    if (directory !== null && require('path').posix.dirname(norm) !== directory) fail('MoreThanOneFolder');
    const dataAt = lho + 30 + buf.readUInt16LE(lho + 26) + buf.readUInt16LE(lho + 28);
    const raw = buf.slice(dataAt, dataAt + csize);
    if (method === 0) out.push(new Uint8Array(raw));
    else if (method === 8) out.push(new Uint8Array(zlib.inflateRawSync(raw)));
    else fail('ExtractFailed', `unsupported compression method ${method}`);
  }
  if (!out.length) fail('NoFiles', 'No dicom data collected');
  return out;
}
/** worker.ts:115-126 fetch(url) + exportResponseBytes: a path or a file:// URL (this Node has no fetch, the machines no network) */
function fetchBytes(url) {
  if (/^file:\/\//.test(url)) return fs.readFileSync(new (require('url').URL)(url));
  if (/^[a-z][a-z0-9+.-]*:\/\//i.test(url)) throw new Error(`fetch is not available in this host: ${url} (read the bytes and call the *Bytes / loadEnv method)`);
  return fs.readFileSync(url);
}
/** hdr.rs:23-36: encoded environment map -> { floats, width, height } with row 0 = top.  Radiance RGBE only. */
function decodeEnvironment(b) {
  if (b.length >= 4 && b.readUInt32LE(0) === 0x01312f76) throw new Error("OpenEXR decode is outside this build's scope (hdr.rs uses the `image` crate's exr decoder): decode the map elsewhere and pass {width, height, floats} to setupEnv()");
  const head = b.toString('latin1', 0, 10);
  if (!head.startsWith('#?RADIANCE') && !head.startsWith('#?RGBE')) throw new Error('unrecognised environment map format (expected Radiance RGBE; decoded floats go to setupEnv())');
  let pos = b.indexOf('\n\n') + 2;
  if (!b.toString('latin1', 0, pos).includes('FORMAT=32-bit_rle_rgbe')) throw new Error('Radiance map: only FORMAT=32-bit_rle_rgbe is supported');
  const eol = b.indexOf('\n', pos), dims = b.toString('latin1', pos, eol).trim().split(/\s+/);
  if (dims.length !== 4 || dims[0] !== '-Y' || dims[2] !== '+X') throw new Error('Radiance map: only the standard -Y h +X w orientation is supported');
  const h = parseInt(dims[1], 10), w = parseInt(dims[3], 10);
  let p = eol + 1;
  const px = new Uint8Array(w * h * 4);
  for (let y = 0; y < h; ++y) {
    if (w >= 8 && w < 32768 && b[p] === 2 && b[p + 1] === 2 && ((b[p + 2] << 8) | b[p + 3]) === w) {
      p += 4;
      for (let ch = 0; ch < 4; ++ch) for (let x = 0; x < w;) {
        let n = b[p++];
        const run = n > 128; if (run) n -= 128;
        // a zero-length run never advances; a run past the scanline or the buffer is a corrupt file (the image crate errors too)
        if (n === 0 || x + n > w || p + (run ? 1 : n) > b.length) throw new Error('Radiance map: corrupt run-length data');
        if (run) { const v = b[p++]; for (let k = 0; k < n; ++k) px[(y * w + x + k) * 4 + ch] = v; } else { for (let k = 0; k < n; ++k) px[(y * w + x + k) * 4 + ch] = b[p++]; }
        x += n;
      }
    } else { if (p + 4 * w > b.length) throw new Error('Radiance map: pixel data ends early'); for (let k = 0; k < 4 * w; ++k) px[y * w * 4 + k] = b[p++]; }
  }
  const floats = new Float32Array(w * h * 4);
  for (let i = 0; i < w * h; ++i) {
    const e = px[4 * i + 3], s = e > 0 ? Math.pow(2, e - 136) : 0;
    floats[4 * i] = Math.fround(px[4 * i] * s); floats[4 * i + 1] = Math.fround(px[4 * i + 1] * s); floats[4 * i + 2] = Math.fround(px[4 * i + 2] * s); floats[4 * i + 3] = 1;
  }
  return { floats, width: w, height: h };
}

// ---- the argument checks several methods share; `who` is the calling method, the prefix of its messages ------------------
const F32_MAX = 3.4028234663852886e38;
const ints = (v) => Array.isArray(v) && v.length === 3 && v.every(Number.isInteger);
/** [lo, hi] as float32 with lo <= hi; hi = Infinity stands for the largest float32 */
function checkBand(who, lo, hi) {
  const l32 = Math.fround(lo), h32 = hi === Infinity ? F32_MAX : Math.fround(hi);
  if (!Number.isFinite(l32) || !Number.isFinite(h32)) throw new Error(`${who}: lo and hi must be finite (hi may be Infinity)`);
  if (l32 > h32) throw new Error(`${who}: lo = ${lo} > hi = ${hi}`);
  return [l32, h32];
}
/** [lo, hi] of box = [[x0, y0, z0], [x1, y1, z1]], inclusive voxel indices inside the index extent e; null: all of it */
function checkBox(who, box, e) {
  const [blo, bhi] = box === null ? [[0, 0, 0], e.map(x => x - 1)] : box;
  if (!ints(blo) || !ints(bhi) || ![0, 1, 2].every(a => blo[a] >= 0 && blo[a] <= bhi[a] && bhi[a] < e[a]))
    throw new Error(`${who}: box ${JSON.stringify(box)} is empty or outside the index extent ${e}`);
  return [blo, bhi];
}
/** the voxel v = [x, y, z] inside the index extent e; `name` is what the method calls it */
const checkVoxel = (who, name, v, e) => { if (!ints(v) || !v.every((x, a) => x >= 0 && x < e[a])) throw new Error(`${who}: ${name} ${v} is outside the index extent ${e}`); };
const checkConnectivity = (who, c) => { if (c !== 6 && c !== 26) throw new Error(`${who}: connectivity must be 6 or 26, not ${c}`); };
/** the voxel spacing [sx, sy, sz] as three finite float32 > 0; null: the norms of the columns of the grid transform (column
 *  major), the grid's own units (mm for DICOM) */
function checkSpacing(who, sp, transform) {
  if (sp === null) sp = [0, 1, 2].map(a => Math.sqrt(transform[4 * a] ** 2 + transform[4 * a + 1] ** 2 + transform[4 * a + 2] ** 2));
  const t = Array.isArray(sp) || ArrayBuffer.isView(sp) ? Array.from(sp, x => (typeof x === 'number' ? Math.fround(x) : NaN)) : [];
  if (t.length !== 3 || !t.every(x => Number.isFinite(x) && x > 0)) throw new Error(`${who}: spacing must be three finite numbers > 0 (x, y, z), not ${sp}`);
  return t;
}
/** a radius or a cap r > 0 as float32; finite unless allowInf (maxDistance = Infinity: no cap) */
function checkDistance(who, name, r, allowInf) {
  const r32 = typeof r === 'number' ? Math.fround(r) : NaN;
  if (!(r32 > 0) || (!Number.isFinite(r32) && !(allowInf && r === Infinity)))
    throw new Error(`${who}: ${name} must be ${allowInf ? '> 0 (Infinity: no cap)' : 'finite and > 0'}, not ${r}`);
  return r32;
}
/** a slot of the segment store: an integer 0 .. SEGMENT_SLOTS - 1; `name` is what the method calls it */
function checkSlot(who, s, name = 'slot') {
  if (!Number.isInteger(s) || s < 0 || s >= SEGMENT_SLOTS) throw new Error(`${who}: ${name} must be an integer 0 .. ${SEGMENT_SLOTS - 1}, not ${s}`);
  return s;
}
/** the slot list of a label map: 1 .. SEGMENT_SLOTS different slots, in the order given */
function checkSlots(who, ss) {
  const t = Array.isArray(ss) || ArrayBuffer.isView(ss) ? Array.from(ss) : null;
  if (t === null || t.length < 1 || t.length > SEGMENT_SLOTS) throw new Error(`${who}: slots must list 1 .. ${SEGMENT_SLOTS} slots, not ${t === null ? ss : t.length}`);
  t.forEach(s => checkSlot(who, s, 'slots: every entry'));
  if (new Set(t).size !== t.length) throw new Error(`${who}: slots must not list a slot twice, as ${t} does`);
  return Uint32Array.from(t);
}
/** [VxHistSource, slot] of a histogram's source: 'volume', 'segment' or an integer slot of the segment store */
function checkHistSource(who, source) {
  if (source === 'volume') return [0, 0];
  if (source === 'segment') return [1, 0];
  if (!Number.isInteger(source) || source < 0 || source >= SEGMENT_SLOTS)
    throw new Error(`${who}: source must be 'volume', 'segment' or an integer slot 0 .. ${SEGMENT_SLOTS - 1}, not ${source}`);
  return [2, source];
}
function checkHistBins(who, bins) {
  if (!Number.isInteger(bins) || bins < 1 || bins > HIST_MAX_BINS) throw new Error(`${who}: bins must be an integer 1 .. ${HIST_MAX_BINS}, not ${bins}`);
  return bins;
}
/** [lo, hi] of a histogram's range as float32 with lo < hi, both finite */
function checkHistRange(who, r) {
  const t = Array.isArray(r) && r.length === 2 ? r.map(x => (typeof x === 'number' ? Math.fround(x) : NaN)) : [NaN, NaN];
  if (!Number.isFinite(t[0]) || !Number.isFinite(t[1]) || !(t[0] < t[1])) throw new Error(`${who}: range must be (lo, hi), two finite numbers with lo < hi, not ${r}`);
  return t;
}
/** the 0-based ranks of an order statistic over n values: a sequence of integers 0 .. n - 1 */
function checkRanks(who, ks, n = null) {
  const t = Array.isArray(ks) || ArrayBuffer.isView(ks) ? Array.from(ks) : null;
  if (t === null) throw new Error(`${who}: ranks must be a sequence of integers, not ${ks}`);
  for (const k of t) {
    if (n === null && (!Number.isInteger(k) || k < 0)) throw new Error(`${who}: ranks: every entry must be an integer >= 0, not ${k}`);
    if (n !== null && (!Number.isInteger(k) || k < 0 || k >= n)) throw new Error(`${who}: ranks: every entry must be an integer 0 .. ${n - 1} (the region has ${n} voxels), not ${k}`);
  }
  return t;
}
/** [values, scalar] of a percentile argument: a number or a sequence of numbers in [0, 100] */
function checkPercentiles(who, q) {
  const scalar = typeof q === 'number';
  const t = scalar ? [q] : (Array.isArray(q) || ArrayBuffer.isView(q) ? Array.from(q) : [null]);
  if (!t.every(x => typeof x === 'number' && x >= 0 && x <= 100)) throw new Error(`${who}: q must be a number or a sequence of numbers in [0, 100], not ${q}`);
  return [t, scalar];
}
/** Otsu's split of a histogram: the k in 0 .. B - 2 that maximises w0 w1 (mu0 - mu1)^2 over the classes bins 0 .. k and
 *  k + 1 .. B - 1, bin centres standing for the bins, ties to the lowest k; -1 with fewer than two non-empty bins (the Python
 *  host's otsu_split, operation for operation) */
function otsuSplit(counts, edges) {
  const B = counts.length;
  if (counts.reduce((n, c) => n + (c !== 0 ? 1 : 0), 0) < 2) return -1;
  const cw = new Float64Array(B), cs = new Float64Array(B);
  let w = 0, s = 0;
  for (let k = 0; k < B; ++k) { w += counts[k]; s += counts[k] * ((edges[k] + edges[k + 1]) / 2); cw[k] = w; cs[k] = s; }
  let best = 0, bestVar = -1;
  for (let k = 0; k + 1 < B; ++k) {
    const w0 = cw[k], w1 = cw[B - 1] - w0, s0 = cs[k], s1 = cs[B - 1] - s0;
    const v = w0 > 0 && w1 > 0 ? w0 * w1 * (s0 / w0 - s1 / w1) ** 2 : 0;
    if (v > bestVar) { best = k; bestVar = v; }
  }
  return best;
}
/** the VxSliceParams block of a slice spec with reduce = mean, no display and the window [0, 1] */
function sliceParams(who, origin, du, dv, dn, [W, H], slabSamples) {
  if (!(W >= 1 && W <= 16384 && H >= 1 && H <= 16384)) throw new Error(`${who}: size must be 1 .. 16384 per side, not ${W} x ${H}`);
  const p = new ParamsBlock(SLICE_LAYOUT);
  p.set('origin', origin); p.set('du', du); p.set('dv', dv); p.set('dn', dn);
  p.set('size', [W, H]); p.set('slab_samples', slabSamples); p.set('reduce', 0); p.set('display', 0); p.set('window', [0, 1]);
  return p;
}

let workerFactory = null;
/** registerVolxelComponents (viewer.ts:1455-1462): keeps the worker factory and names the component classes.  The four
 *  widget elements are browser UI without a counterpart here; the renderer calls the native preprocessor in-process. */
function registerVolxelComponents(worker) {
  workerFactory = worker || null;
  return { 'volxel-3d-viewer': Volxel3DDicomRenderer };
}

class Volxel3DDicomRenderer {
  /** width, height: the canvas.  lowResPreview reproduces the viewer's interactive sizing
   *  (settings.resolutionFactor and the 0.33 ramp of viewer.ts:1167-1188); off = full-size frames.
   *  devices: render one image on several GPUs (a device group, member i renders shard i; an id may repeat) in
   *  place of the one `device`; every other call is the same. */
  constructor({ width = 1920, height = 1080, device, devices, layout, lowResPreview = false } = {}) {
    if (devices !== undefined && device !== undefined) throw new Error('pass either device or devices, not both');
    // throws when no GPU is visible
    this.ctx = devices !== undefined ? native.createGroup(devices) : native.create(device === undefined ? 0 : device);
    this.devices = devices !== undefined ? devices.slice() : null;
    this.canvasWidth = width; this.canvasHeight = height;
    this.width = width; this.height = height;    // current render size
    this.lowResPreview = lowResPreview; this.resolutionFactor = 1.0; // viewer.ts:131
    this.settings = { // viewer.ts:147-163 + [build] DVR parameters
      densityMultiplier: 1, maxSamples: 2000, debugHits: false, volumeClipMin: [0, 0, 0], volumeClipMax: [1, 1, 1],
      showEnvironment: true, useEnv: true, lightDir: [-1, -1, -1].map(v => v / Math.sqrt(3)), syncLightDir: false,
      bounces: 3, gamma: 2.2, exposure: 5.5, sampleRange: [0, 1], renderMode: 'default', resolutionFactor: 1,
      dvrStepVoxels: 0.5, dvrErtEpsilon: 1e-4, dvrJitter: false, dvrMaxSteps: 1 << 20, dvrSkipEmpty: true, phong: [0.3, 0.7, 0.4, 32],
      dvrShadowStride: 0,   // shadowed DVR: 0 off, 1 / 2 / 4 light-grid stride (volxel_hip.h VxParams.dvr_shadow_stride)
    };
    this.camera = new Camera(1);                  // viewer.ts:418
    this.environment = null;
    this.frameIndex = 0;
    this.densityScale = 1;
    this.volume = null;
    if (layout !== undefined) native.setLayout(this.ctx, layout);
    native.resize(this.ctx, width, height);
    this.setEnvironment(Environment.default());   // viewer.ts:372-374
    const tf = generateTransferFunction([{ color: [1, 1, 1, 0], stop: 0 }, { color: [1, 1, 1, 1], stop: 1 }]);
    this.changeTransferFunc(tf.data, tf.length);  // viewer.ts:377-385
  }
  setEnvironment(env) { // viewer.ts:1073-1078; null removes the map (directional light only)
    if (env) native.uploadEnvironment(this.ctx, env.floats, env.width, env.height);
    else native.uploadEnvironment(this.ctx, null, 0, 0);
    this.environment = env || null;
    this.restartRendering();
  }
  get envStrength() { return this.environment ? this.environment.strength : (this._envStrength === undefined ? 1 : this._envStrength); }
  set envStrength(v) { this._envStrength = v; if (this.environment) this.environment.strength = v; }
  dispose() { if (this.ctx) { native.destroy(this.ctx); this.ctx = null; } }

  get renderMode() { return this.settings.renderMode; }
  set renderMode(to) {
    if (!(to in RenderMode)) throw new Error(`Unrecognized render mode provided: ${to}`);
    this.settings.renderMode = to; this.restartRendering();
  }

  /** restartFromFiles (viewer.ts:963-975): DICOM slice paths (or Uint8Arrays) in stacking order */
  restartFromFiles(files, threads = 0) {
    this.restartFromBytes(files.map(f => (typeof f === 'string' ? new Uint8Array(fs.readFileSync(f)) : f)), threads);
  }
  /** restartFromZip (viewer.ts:977-989): a ZIP of DICOM slices (Buffer / Uint8Array / path), folder rule of zip.rs:54-70 */
  restartFromZip(zip, threads = 0) {
    this.restartFromBytes(readZipSlices(typeof zip === 'string' ? fs.readFileSync(zip) : Buffer.from(zip.buffer || zip, zip.byteOffset || 0, zip.byteLength)), threads);
  }
  /** restartFromZipUrl (viewer.ts:991-1003, worker.ts:115-118) */
  restartFromZipUrl(url, threads = 0) { this.restartFromZip(fetchBytes(url), threads); }
  /** restartFromURLs (viewer.ts:1005-1017, worker.ts:120-123): one slice per URL, in the order given */
  restartFromURLs(urls, threads = 0) { this.restartFromBytes(urls.map(u => new Uint8Array(fetchBytes(u))), threads); }
  /** loadEnv (viewer.ts:1019-1033, worker.ts:77-90, hdr.rs:23-36): Radiance RGBE is decoded, OpenEXR is refused */
  loadEnv(bytes) { this.setupEnv(decodeEnvironment(Buffer.from(bytes.buffer || bytes, bytes.byteOffset || 0, bytes.byteLength))); }
  /** loadEnvFromUrl (viewer.ts:1035-1040) */
  loadEnvFromUrl(url) { this.loadEnv(fetchBytes(url)); }
  /** maybeSyncLight (viewer.ts:789-795): lightDir = -(view - pos), normalised by the direction widget it is assigned to
   *  (cubeDirection.ts:177-206).  Called after a camera rotation and by the backlight toggle -- not by restoreSettings,
   *  exactly as in the reference. */
  maybeSyncLight() {
    if (!this.settings.syncLightDir) return;
    const d = V.sub(this.camera.pos, this.camera.view), n = V.len(d);
    if (n > 0) this.settings.lightDir = V.scale(d, 1 / n);
  }
  rotateCamera(by) { this.camera.rotateAroundView(by); this.maybeSyncLight(); this.restartRendering(); } // viewer.ts:443-449
  get syncLightDir() { return this.settings.syncLightDir; }
  set syncLightDir(on) { this.settings.syncLightDir = !!on; this.maybeSyncLight(); this.restartRendering(); } // viewer.ts:543-551
  /** setupEnv (viewer.ts:1073-1078): { width, height, floats } with row 0 = top */
  setupEnv(env) { this.setEnvironment(new Environment(env.floats, env.width, env.height)); }
  /** the same once the files are in memory: one Uint8Array per slice (worker.ts:101-104) */
  restartFromBytes(files, threads = 0) {
    this.setupFromGrid(native.readDicomsToGrid(files, threads));
  }

  /** the same for an already decoded u16 stack */
  restartFromVoxels(voxels, dims, spacing = [1, 1, 1], maxValue = 0, threads = 0) {
    this.setupFromGrid(native.buildBrickGrid(voxels, dims, spacing, maxValue, threads));
  }

  setupFromGrid(grid) { // viewer.ts:1080-1145
    this.densityScale = 1;
    this.settings.volumeClipMax = [1, 1, 1]; this.settings.volumeClipMin = [0, 0, 0];
    const g = Array.from(grid.transform);
    const e = grid.indexExtent;
    const lo = M.apply(g, [0, 0, 0, 1]).slice(0, 3), hi = M.apply(g, [e[0], e[1], e[2], 1]).slice(0, 3);
    const ext = hi.map((v, i) => v - lo[i]);
    const size = Math.max(ext[0], Math.max(ext[1], ext[2]));
    let t = M.identity();
    if (size !== 1) {
      t = M.mul(M.scale([1 / size, 1 / size, 1 / size]), M.translate(lo.map((v, i) => -v - ext[i] * 0.5)));
      this.densityScale *= size;
    }
    this.volume = { grid: { transform: g, indexExtent: e, minMaj: grid.minMaj }, transform: t };
    native.uploadVolume(this.ctx, grid);
    this.restartRendering();
  }

  changeTransferFunc(data, length) { // viewer.ts:1147-1153
    native.uploadTransfer(this.ctx, data, length);
    this.frameIndex = 0;
  }
  restartRendering() {                          // viewer.ts:1155-1181
    if (this.lowResPreview) { this.resolutionFactor = 0.33; this.resizeFramebuffersToCanvas(); }
    this.frameIndex = 0;
  }
  resizeFramebuffersToCanvas() {                // viewer.ts:925-949
    const f = this.lowResPreview ? this.resolutionFactor * this.settings.resolutionFactor : 1.0;
    const w = Math.max(1, Math.floor(this.canvasWidth * f)), h = Math.max(1, Math.floor(this.canvasHeight * f));
    if (w !== this.width || h !== this.height) { this.width = w; this.height = h; native.resize(this.ctx, w, h); }
  }

  restoreSettings(s) { // viewer.ts:704-713 (+ transfer/display/lighting closures)
    if (s.version !== 'v3') throw new Error(`Unsupported Settings Format Version: ${s.version}`);
    this.settings.densityMultiplier = s.transfer.densityMultiplier;
    this.settings.sampleRange = s.transfer.histogramRange.slice();
    if (s.transfer.transfer.type === 'color_stops') {
      const tf = generateTransferFunction(s.transfer.transfer.colors);
      this.changeTransferFunc(tf.data, tf.length);
    } else {
      this.changeTransferFunc(new Float32Array(s.transfer.transfer.colors.flat()), s.transfer.transfer.colors.length);
    }
    Object.assign(this.settings, {
      bounces: s.display.bounces, maxSamples: s.display.samples, gamma: s.display.gamma, exposure: s.display.exposure,
      debugHits: s.display.debugHits, renderMode: s.display.renderMode, resolutionFactor: s.display.resolutionFactor,
      showEnvironment: s.lighting.showEnv, useEnv: s.lighting.useEnv, syncLightDir: s.lighting.syncLightDir,
      lightDir: s.lighting.lightDir.slice(), volumeClipMax: s.other.clipMax.slice(), volumeClipMin: s.other.clipMin.slice(),
    });
    this.envStrength = s.lighting.envStrength;
    this.camera.pos = s.other.cameraPos.slice(); this.camera.view = s.other.cameraLookAt.slice();
    this.restartRendering();
  }

  densityTransform() { return M.mul(this.volume.transform, this.volume.grid.transform); } // volume.ts:14-16
  /** the index-from-world matrix bindUniforms sends as density_transform_inv (doubles; the uniform holds them as float32) */
  densityTransformInv() { return M.invert(this.densityTransform()); }

  bindUniforms() { // viewer.ts:1295-1357 + scene.ts:53-56
    if (!this.volume) throw new Error('Trying to bind uniforms without a volume.');
    const p = new ParamsBlock(), s = this.settings;
    const view = this.camera.viewMatrix(), proj = this.camera.projMatrix(this.width / this.height);
    p.set('camera_view', view); p.set('camera_proj', proj);
    p.set('camera_view_inv', M.invert(M.f32(view))); p.set('camera_proj_inv', M.invert(M.f32(proj)));
    p.set('camera_ortho', this.camera.orthoHalfHeight !== null ? 1 : 0);
    const combined = this.densityTransform();
    const e = this.volume.grid.indexExtent;
    const lo = M.apply(combined, [0, 0, 0, 1]), hi = M.apply(combined, [e[0], e[1], e[2], 1]);
    p.set('volume_aabb_min', [0, 1, 2].map(i => lo[i] + (hi[i] - lo[i]) * s.volumeClipMin[i]));
    p.set('volume_aabb_max', [0, 1, 2].map(i => lo[i] + (hi[i] - lo[i]) * s.volumeClipMax[i]));
    const [mn, maj] = this.volume.grid.minMaj, k = this.densityScale * s.densityMultiplier;
    p.set('volume_min', mn * k); p.set('volume_maj', maj * k); p.set('volume_inv_maj', 1 / (maj * k));
    p.set('volume_albedo', [0.9, 0.9, 0.9]); p.set('volume_phase_g', 0); p.set('volume_density_scale', k);
    p.set('density_transform', combined); p.set('density_transform_inv', this.densityTransformInv());
    p.set('sample_range', s.sampleRange);
    p.set('light_dir', s.lightDir); p.set('env_strength', this.envStrength);
    p.set('show_environment', s.showEnvironment ? 1 : 0); p.set('use_env', s.useEnv && this.environment ? 1 : 0); p.set('bounces', s.bounces);
    p.set('res', [this.width, this.height]); p.set('debug_hits', s.debugHits ? 1 : 0);
    p.set('render_mode', RenderMode[s.renderMode]);
    p.set('dvr_step_voxels', s.dvrStepVoxels); p.set('dvr_ert_tau', -Math.log(s.dvrErtEpsilon));
    p.set('dvr_jitter', s.dvrJitter ? 1 : 0); p.set('dvr_max_steps', s.dvrMaxSteps); p.set('dvr_skip_empty', s.dvrSkipEmpty ? 1 : 0);
    p.set('dvr_shadow_stride', s.dvrShadowStride | 0);
    const f = Math.fround;
    const fp = f(f(1) / f(f(4) * f(Math.PI)));                         // utils.glsl:121-124, g = 0
    const mis = s.showEnvironment ? f(f(1) / f(f(1) + f(fp * fp))) : f(1); // utils.glsl:104
    const gain = f(f(f(f(0.9) * mis) * fp) * f(f(this.envStrength) * f(4.01)));
    p.set('dvr_gain', [gain, gain, gain]);
    p.set('phong_ka', s.phong[0]); p.set('phong_kd', s.phong[1]); p.set('phong_ks', s.phong[2]);
    p.set('phong_shininess', s.phong[3]);
    p.set('shard_rank', 0); p.set('shard_count', 1);
    native.setParams(this.ctx, p.buffer);
    this.params = p;
    return p;
  }

  /** frames accumulation samples, up to inFlight of them per launch (vx_render_frames: same bits as one launch per
   *  frame, 1.6x the speed at 32) */
  render(frames = 1, inFlight = 32) { // viewer.ts:1183-1293
    const weight = f => (f < LOW_RES_DURATION ? 0 : (f - LOW_RES_DURATION) / (f - LOW_RES_DURATION + 1)); // viewer.ts:1356
    let bound = false;
    for (let i = 0; i < frames && this.frameIndex <= this.settings.maxSamples;) {
      if (this.lowResPreview && this.frameIndex >= LOW_RES_DURATION && this.resolutionFactor !== 1.0) {
        this.resolutionFactor = 1.0; this.resizeFramebuffersToCanvas(); bound = false; // viewer.ts:1185-1188
      }
      if (!bound) { this.bindUniforms(); bound = true; }
      const f = this.frameIndex;
      const ramp = this.lowResPreview && f < LOW_RES_DURATION;   // the size changes at LOW_RES_DURATION
      let n = Math.min(frames - i, this.settings.maxSamples + 1 - f);
      if (ramp) n = Math.min(n, LOW_RES_DURATION - f);
      if (inFlight > 1 && n > 1) {
        const w = new Float32Array(n);
        for (let k = 0; k < n; ++k) w[k] = weight(f + k);
        native.renderFrames(this.ctx, f, w, inFlight);
      } else {
        n = 1;
        native.renderFrame(this.ctx, f, weight(f));
      }
      this.frameIndex += n; i += n;
    }
  }
  /** startBenchmark (viewer.ts:856-890) + the result record of viewer.ts:1229-1241.  `volumes` maps an
   *  entry's "zip" string to a brick-grid message (container I/O is outside the path). */
  startBenchmark(collection, volumes = {}) {
    if (!collection || !Array.isArray(collection.sharedSettings) || !Array.isArray(collection.benchmarks)) throw new Error('Malformed benchmark collection.');
    const results = [], savedPreview = this.lowResPreview;
    this.lowResPreview = true;                    // the viewer's framebuffer sizing is part of the scenario
    try {
      for (const b of collection.benchmarks) {
        if (b.zip !== undefined) {
          if (!volumes[b.zip]) throw new Error(`benchmark volume not provided: ${b.zip}`);
          this.setupFromGrid(volumes[b.zip]);
        }
        if (b.env !== undefined) throw new Error('benchmark entry asks for an environment map URL; pass the decoded map with setEnvironment() before the run');
        this.restoreSettings(typeof b.settings === 'number' ? collection.sharedSettings[b.settings] : b.settings);
        if (b.renderMode) this.renderMode = b.renderMode;
        this.restartRendering();
        let total = 0;
        while (this.frameIndex <= this.settings.maxSamples) {   // viewer.ts:1194
          const t0 = process.hrtime.bigint();
          this.render(1); this.finish();                          // viewer.ts:1213-1218
          total += Number(process.hrtime.bigint() - t0) / 1e6;
        }
        const rf = this.settings.resolutionFactor;
        results.push(JSON.parse(JSON.stringify({
          name: b.name, settings: this.settings, timePerSample: total / this.frameIndex, totalTime: total,
          viewport: [0, 0, rf * this.canvasWidth, rf * this.canvasHeight],
          device: { platform: process.platform, userAgent: `node ${process.version} / volxel_hip ${native.version()}`,
            hardwareConcurrency: require('os').cpus().length, screen: { width: this.canvasWidth, height: this.canvasHeight, pixelRatio: 1 },
            gpu: { vendor: 'AMD', renderer: this.deviceInfo().name.trim(), version: 'HIP' } },
          timestamp: new Date(),
        })));
      }
    } finally {
      this.lowResPreview = savedPreview;
      if (!savedPreview) { this.resolutionFactor = 1.0; this.resizeFramebuffersToCanvas(); }
    }
    return results;
  }
  /** multi-GPU hosts: cost estimate of every 64x64 tile / dealing order of the tiles (volxel_hip.h) */
  probeTileCosts() {
    this.bindUniforms();
    const n = Math.ceil(this.width / 64) * Math.ceil(this.height / 64), out = new Uint32Array(n);
    native.probeTileCosts(this.ctx, out);
    return out;
  }
  setTileOrder(perm) { native.setTileOrder(this.ctx, perm || null); this.restartRendering(); }
  deviceInfo() { return native.deviceInfo(this.ctx); }
  finish() { native.finish(this.ctx); }
  readAccum() { const o = new Float32Array(this.width * this.height * 4); native.readAccum(this.ctx, o); return o; }
  readDisplay() { // the blit to the canvas (NEAREST, viewer.ts:310-311,1253-1265)
    const o = new Uint8Array(this.canvasWidth * this.canvasHeight * 4);
    native.readDisplayScaled(this.ctx, o, this.canvasWidth, this.canvasHeight, this.settings.exposure, this.settings.gamma);
    return o;
  }
  counters() { return native.getCounters(this.ctx); }
  /** shadowed DVR (settings.dvrShadowStride): light-grid builds, light-march samples and time of the last build */
  shadowStats() { return native.shadowStats(this.ctx); }
  /** the last light grid built: node transmittances, x fastest */
  readShadowGrid() { return native.readShadowGrid(this.ctx); }
  resetCounters() { native.resetCounters(this.ctx); }

  /** index-space planes through voxel centres, one pixel per voxel (Python: volxel_amd.mpr); patient orientation is not
   *  modelled.  Each returns a slice spec for slice(). */
  sliceExtent() {
    if (!this.volume) throw new Error('Trying to slice without a volume.');
    return this.volume.grid.indexExtent;
  }
  axial(k) { const e = this.sliceExtent(); return sliceSpec('k', k, e[2], [0, 0, k], [1, 0, 0], [0, 1, 0], [0, 0, 1], [e[0], e[1]]); }
  coronal(j) { const e = this.sliceExtent(); return sliceSpec('j', j, e[1], [0, j, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0], [e[0], e[2]]); }
  sagittal(i) { const e = this.sliceExtent(); return sliceSpec('i', i, e[0], [i, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0], [e[1], e[2]]); }
  /** vx_slice: { origin, du, dv, dn (cell frame), size: [W, H], slabSamples = 1, reduce = 'mean' | 'max' | 'min',
   *  display = null | 'grey' | 'tf', window = [black, white] (grey only) } -> { values: Float32Array (W*H, row 0 = y = 0),
   *  rgba8: Uint8Array (W*H*4) | null }.  Binds the current uniforms first. */
  slice({ origin, du, dv, dn, size, slabSamples = 1, reduce = 'mean', display = null, window = null }) {
    if (!(reduce in SliceReduce)) throw new Error(`slice: reduce must be 'mean', 'max' or 'min', not ${reduce}`);
    if (display !== null && !(display in SliceDisplay)) throw new Error(`slice: display must be null, 'grey' or 'tf', not ${display}`);
    if (display === 'grey' && !(window && window.length === 2 && Math.fround(window[1]) > Math.fround(window[0])))
      throw new Error('slice: display grey needs window = [black, white] with black < white');
    if (display !== 'grey' && window !== null) throw new Error('slice: window applies to display grey only');
    const p = sliceParams('slice', origin, du, dv, dn, size, slabSamples), [W, H] = size;
    p.set('reduce', SliceReduce[reduce]); p.set('display', display === null ? 0 : SliceDisplay[display]);
    if (display === 'grey') p.set('window', window);
    this.bindUniforms();
    const values = new Float32Array(W * H), rgba8 = display === null ? null : new Uint8Array(W * H * 4);
    native.slice(this.ctx, p.buffer, values, rgba8);
    return { values, rgba8 };
  }
  /** the last slice: W*H*N samples and its kernel time (vx_slice_stats) */
  sliceStats() { return native.sliceStats(this.ctx); }

  /** vx_isosurface: the shaded first hit of density iso.  opts: { color = [1, 1, 1], phong = settings.phong
   *  ([ka, kd, ks, shininess]), refine = 8, skip = true, window = null ([x0, y0, x1, y1] of the render size, GL rows) }
   *  -> { rgba, hit: Float32Array (4 floats per window pixel, row 0 = y0), width, height }; hit = (world x, y, z, t),
   *  (0, 0, 0, -1) on a miss.  Binds the current uniforms first. */
  isosurface(iso, { color = [1, 1, 1], phong = null, refine = 8, skip = true, window = null } = {}) {
    const fin = (v, n) => Array.isArray(v) && v.length === n && v.every((x) => Number.isFinite(Math.fround(x)));
    if (!Number.isFinite(Math.fround(iso))) throw new Error(`isosurface: iso must be finite, not ${iso}`);
    if (!fin(color, 3)) throw new Error('isosurface: color must be three finite numbers');
    const ph = phong === null ? this.settings.phong : phong;
    if (!fin(ph, 4) || ph[3] < 0) throw new Error('isosurface: phong must be [ka, kd, ks, shininess], finite, shininess >= 0');
    if (!Number.isInteger(refine) || refine < 0 || refine > 16) throw new Error(`isosurface: refine must be an integer 0 .. 16, not ${refine}`);
    if (typeof skip !== 'boolean') throw new Error('isosurface: skip must be true or false');
    this.bindUniforms();
    const W = this.width, H = this.height;
    const [x0, y0, x1, y1] = window === null ? [0, 0, W, H] : window;
    if (![x0, y0, x1, y1].every(Number.isInteger) || !(x0 >= 0 && x0 < x1 && x1 <= W && y0 >= 0 && y0 < y1 && y1 <= H))
      throw new Error(`isosurface: window ${window} is empty or outside the render size ${W} x ${H}`);
    const p = new ParamsBlock(ISO_LAYOUT);
    p.set('iso', iso); p.set('color', color);
    p.set('ka', ph[0]); p.set('kd', ph[1]); p.set('ks', ph[2]); p.set('shininess', ph[3]);
    p.set('refine', refine); p.set('skip', skip ? 1 : 0); p.set('window', [x0, y0, x1, y1]);
    const n = (x1 - x0) * (y1 - y0);
    const rgba = new Float32Array(4 * n), hit = new Float32Array(4 * n);
    native.isosurface(this.ctx, p.buffer, rgba, hit);
    return { rgba, hit, width: x1 - x0, height: y1 - y0 };
  }
  /** the world point [x, y, z] where the ray of pixel (x, y) (GL rows) first reaches density iso, or null on a miss */
  pick(x, y, iso, { refine = 16 } = {}) {
    const { hit } = this.isosurface(iso, { refine, window: [x, y, x + 1, y + 1] });
    return hit[3] < 0 ? null : [hit[0], hit[1], hit[2]];
  }
  /** the last isosurface: rays, hits, samples, refineSamples, skipped and its kernel time (vx_iso_stats) */
  isoStats() { return native.isoStats(this.ctx); }

  /** vx_segment: the connected component of lo <= d <= hi holding the voxel seed = [x, y, z] (DESIGN.md section 2
   *  "Segmentation").  opts: { hi = Infinity (the largest float32), connectivity = 6 | 26, box = null ([[x0, y0, z0],
   *  [x1, y1, z1]], inclusive; null: the whole volume), maxRounds = 0 (no practical cap) } -> { count, bboxLo, bboxHi, dMin,
   *  dMax, dSum, mean, rounds, converged, brickVisits }.  Binds the current uniforms first. */
  segment(seed, lo, { hi = Infinity, connectivity = 6, box = null, maxRounds = 0 } = {}) {
    const e = this.sliceExtent();
    checkVoxel('segment', 'seed', seed, e);
    const [l32, h32] = checkBand('segment', lo, hi);
    checkConnectivity('segment', connectivity);
    const [blo, bhi] = checkBox('segment', box, e);
    if (!Number.isInteger(maxRounds) || maxRounds < 0 || maxRounds > 4294967295) throw new Error(`segment: maxRounds must be an integer >= 0`);
    const p = new ParamsBlock(SEGMENT_LAYOUT);
    p.set('seed', seed); p.set('lo', l32); p.set('hi', h32); p.set('connectivity', connectivity);
    p.set('box_lo', blo); p.set('box_hi', bhi); p.set('max_rounds', maxRounds);
    this.bindUniforms();
    return this._segmentResult(native.segment(this.ctx, p.buffer));
  }
  /** vx_segment_edit (DESIGN.md section 2 "Segment edits"): op 'dilate' | 'erode' | 'open' | 'close' | 'fill_holes' on the
   *  current segment; opts: { steps = 1 (1 .. 1024; ignored by fill_holes), connectivity = 6 | 26, band = false (dilate only:
   *  grow only into voxels that pass the predicate of the last segment()) } -> what segment() returns, for the edited mask
   *  (rounds and brickVisits: the fill's background flood).  Binds the current uniforms first. */
  segmentEdit(op, { steps = 1, connectivity = 6, band = false } = {}) {
    const i = SEGMENT_EDIT_OPS.indexOf(op);
    if (i < 0) throw new Error(`segmentEdit: op must be one of ${SEGMENT_EDIT_OPS.join(', ')}, not ${op}`);
    checkConnectivity('segmentEdit', connectivity);
    const fill = op === 'fill_holes';
    if (!Number.isInteger(steps) || steps < (fill ? 0 : 1) || steps > (fill ? 1 : 1024))
      throw new Error(`segmentEdit: steps must be an integer ${fill ? '0 .. 1' : '1 .. 1024'} for ${op}, not ${steps}`);
    if (typeof band !== 'boolean') throw new Error(`segmentEdit: band must be a boolean, not ${band}`);
    if (band && op !== 'dilate') throw new Error(`segmentEdit: band is for dilate only, not ${op}`);
    this.bindUniforms();
    return this._segmentResult(native.segmentEdit(this.ctx, i, connectivity, steps, band ? 1 : 0));
  }
  /** vx_segment_margin (DESIGN.md section 2 "Distances and margins"): op 'grow' | 'shrink' | 'open' | 'close' on the current
   *  segment by `radius` in physical units, one exact Euclidean transform per half whatever the radius; opts: { spacing = null
   *  ([sx, sy, sz] in the units of radius; null: the column norms of grid.transform, mm for DICOM), band = false (grow only:
   *  only into voxels that pass the predicate of the last segment() / threshold()) } -> what segment() returns, for the new
   *  mask.  Binds the current uniforms first. */
  segmentMargin(op, radius, { spacing = null, band = false } = {}) {
    this.sliceExtent();
    const i = MARGIN_OPS.indexOf(op);
    if (i < 0) throw new Error(`segmentMargin: op must be one of ${MARGIN_OPS.join(', ')}, not ${op}`);
    const r = checkDistance('segmentMargin', 'radius', radius, false);
    const sp = checkSpacing('segmentMargin', spacing, this.volume.grid.transform);
    if (typeof band !== 'boolean') throw new Error(`segmentMargin: band must be a boolean, not ${band}`);
    if (band && op !== 'grow') throw new Error(`segmentMargin: band is for grow only, not ${op}`);
    this.bindUniforms();
    return this._segmentResult(nativeDistance.segmentMargin(this.ctx, i, r, sp[0], sp[1], sp[2], band ? 1 : 0));
  }
  /** vx_segment_distance: the exact Euclidean distance field of the current segment; opts: { side = 'outside' (how far every
   *  voxel is from the segment) | 'inside' (how far every voxel of the segment is from leaving it), maxDistance = Infinity
   *  (distances above it read Infinity), spacing = null (as segmentMargin) } -> { finite, maxD2, maxDistance, argmax: [x, y, z],
   *  squared(): Float32Array over (z, y, x), distance(): its square roots }.  The segment is not changed. */
  segmentDistance({ side = 'outside', maxDistance = Infinity, spacing = null } = {}) {
    this.sliceExtent();
    const i = DISTANCE_SIDES.indexOf(side);
    if (i < 0) throw new Error(`segmentDistance: side must be one of ${DISTANCE_SIDES.join(', ')}, not ${side}`);
    const cap = checkDistance('segmentDistance', 'maxDistance', maxDistance, true);
    const sp = checkSpacing('segmentDistance', spacing, this.volume.grid.transform);
    this.bindUniforms();
    const r = nativeDistance.segmentDistance(this.ctx, sp[0], sp[1], sp[2], cap, i);
    r.maxDistance = Math.fround(Math.sqrt(r.maxD2));
    r.squared = () => this.distanceField();
    r.distance = () => this.distanceField().map(v => Math.fround(Math.sqrt(v)));
    return r;
  }
  /** the squared distances of the last segmentDistance over (z, y, x), Infinity beyond the cap (vx_distance_read) */
  distanceField() {
    const e = this.sliceExtent();
    const out = new Float32Array(e[0] * e[1] * e[2]);
    nativeDistance.distanceRead(this.ctx, out);
    return out;
  }
  /** the last segmentDistance or segmentMargin: kernels launched and the times of the x, y and z pass and of the compare /
   *  reduction (open and close: summed over their two transforms) */
  distanceStats() { return nativeDistance.distanceStats(this.ctx); }
  /** vx_segment_store (DESIGN.md section 2 "Segment store"): copies the current segment into `slot` (0 .. 31) of the device's
   *  segment store, replacing what it held; the current segment stays */
  storeSegment(slot) {
    this.sliceExtent();
    checkSlot('storeSegment', slot);
    this.bindUniforms();
    nativeSegments.storeSegment(this.ctx, slot);
  }
  /** vx_segment_load: the mask of `slot` becomes the current segment (the slot keeps its copy) -> what segment() returns */
  loadSegment(slot) {
    this.sliceExtent();
    checkSlot('loadSegment', slot);
    this.bindUniforms();
    return this._segmentResult(nativeSegments.loadSegment(this.ctx, slot));
  }
  /** vx_segment_drop: frees `slot`; an empty slot is fine */
  dropSegment(slot) {
    this.sliceExtent();
    checkSlot('dropSegment', slot);
    this.bindUniforms();
    nativeSegments.dropSegment(this.ctx, slot);
  }
  /** the occupied slots, ascending (vx_segment_slots) */
  storedSegments() {
    this.sliceExtent();
    this.bindUniforms();
    const bits = nativeSegments.storedSegments(this.ctx);
    return Array.from({ length: SEGMENT_SLOTS }, (_, k) => k).filter(k => (bits >>> k) & 1);
  }
  /** vx_segment_combine: op 'union' | 'intersect' | 'subtract' | 'xor' on the current segment A and the mask B of `slot`
   *  (A | B, A & B, A & ~B, A ^ B), or 'invert' (~A over the index extent; no slot), in place on the GPU -> what segment()
   *  returns, for the new mask.  Binds the current uniforms first. */
  segmentCombine(op, slot = null) {
    this.sliceExtent();
    const i = COMBINE_OPS.indexOf(op);
    if (i < 0) throw new Error(`segmentCombine: op must be one of ${COMBINE_OPS.join(', ')}, not ${op}`);
    if ((op === 'invert') !== (slot === null)) throw new Error(op === 'invert' ? 'segmentCombine: slot must be null for invert' : `segmentCombine: slot is required for ${op}`);
    if (slot !== null) checkSlot('segmentCombine', slot);
    this.bindUniforms();
    return this._segmentResult(nativeSegments.segmentCombine(this.ctx, i, slot === null ? 0 : slot));
  }
  /** vx_segment_compare: the current segment A against the mask B of `slot`; opts: { hausdorff = true, spacing = null (as
   *  segmentMargin) } -> { countA, countB, countAnd, dice, jaccard (NaN when both sets are empty), and with hausdorff: d2Ab, d2Ba,
   *  hausdorffAb, hausdorffBa (their float32 square roots), hausdorff (the larger), argmaxAb, argmaxBa: [x, y, z]; null
   *  without }.  Neither mask is changed. */
  segmentCompare(slot, { hausdorff = true, spacing = null } = {}) {
    this.sliceExtent();
    checkSlot('segmentCompare', slot);
    if (typeof hausdorff !== 'boolean') throw new Error(`segmentCompare: hausdorff must be a boolean, not ${hausdorff}`);
    const sp = checkSpacing('segmentCompare', spacing, this.volume.grid.transform);
    this.bindUniforms();
    const r = nativeSegments.segmentCompare(this.ctx, slot, hausdorff ? 1 : 0, sp[0], sp[1], sp[2]);
    const sum = r.countA + r.countB;
    r.dice = sum ? 2 * r.countAnd / sum : NaN;
    r.jaccard = sum ? r.countAnd / (sum - r.countAnd) : NaN;
    if (hausdorff) {
      r.hausdorffAb = Math.fround(Math.sqrt(r.d2Ab));
      r.hausdorffBa = Math.fround(Math.sqrt(r.d2Ba));
      r.hausdorff = Math.max(r.hausdorffAb, r.hausdorffBa);
    } else {
      for (const k of ['d2Ab', 'd2Ba', 'argmaxAb', 'argmaxBa', 'hausdorffAb', 'hausdorffBa', 'hausdorff']) r[k] = null;
    }
    return r;
  }
  /** vx_segments_labelmap: the label map of the listed slots -> { labels: Uint8Array over (z, y, x), k + 1 where slots[k] is the
   *  first listed slot that holds the voxel and 0 where none does; overlaps: the voxels more than one listed slot holds } */
  segmentsLabelmap(slots) {
    const e = this.sliceExtent();
    const list = checkSlots('segmentsLabelmap', slots);
    this.bindUniforms();
    const labels = new Uint8Array(e[0] * e[1] * e[2]);
    const overlaps = nativeSegments.segmentsLabelmap(this.ctx, list, labels);
    return { labels, overlaps };
  }
  _histogramParams(who, source, box) {
    const e = this.sliceExtent();
    const [src, slot] = checkHistSource(who, source), [blo, bhi] = checkBox(who, box, e);
    const p = new ParamsBlock(HISTOGRAM_LAYOUT);
    p.set('source', src); p.set('slot', slot); p.set('box_lo', blo); p.set('box_hi', bhi);
    return p;
  }
  /** vx_histogram, LINEAR (DESIGN.md section 2 "Histograms"): the density histogram and the moments of a region on the GPU.
   *  opts: { bins = 256 (1 .. 4096), range = [0, 1] ([lo, hi]; a density equal to hi lands in the last bin), source = 'volume' |
   *  'segment' | an integer slot of the segment store, box = null ([[x0, y0, z0], [x1, y1, z1]], inclusive; null: the whole
   *  index extent) } -> { counts: Float64Array, edges: Float64Array (nominal: lo + k (hi - lo) / bins), below, above, count,
   *  dMin, dMax, dSum, dSum2, mean, std (population; NaN when the region is empty) }.  Binds the current uniforms first; changes
   *  nothing. */
  histogram({ bins = 256, range = [0, 1], source = 'volume', box = null } = {}) {
    const p = this._histogramParams('histogram', source, box);
    const B = checkHistBins('histogram', bins), [lo, hi] = checkHistRange('histogram', range);
    p.set('rule', 0); p.set('bins', B); p.set('lo', lo); p.set('hi', hi); p.set('moments', 1);
    this.bindUniforms();
    const counts = new Float64Array(B);
    const r = nativeHistogram.histogram(this.ctx, p.buffer, counts);
    r.counts = counts;
    r.edges = Float64Array.from({ length: B + 1 }, (_, k) => lo + k * (hi - lo) / B);
    const n = r.count;
    r.mean = n ? r.dSum / n : NaN;
    r.std = n ? Math.sqrt(Math.max(0, (r.dSum2 - r.dSum * r.dSum / n) / n)) : NaN;
    return r;
  }
  /** the radix select behind densityOrderStatistic and densityPercentile: ranksOf(n) -> the ranks, given the size of the region
   *  from the first pass, which all ranks share (as they share every later pass with the same prefix) */
  _orderStatistics(p, ranksOf) {
    p.set('rule', 1); p.set('moments', 0);
    this.bindUniforms();
    const seen = new Map();
    const countsOf = (pb, b, prefix) => {
      const key = `${pb}:${prefix}`;
      if (!seen.has(key)) {
        p.set('prefix', prefix); p.set('prefix_bits', pb); p.set('key_bits', b);
        const counts = new Float64Array(2 ** b);
        const r = nativeHistogram.histogram(this.ctx, p.buffer, counts);
        seen.set(key, { counts, below: r.below, count: r.count });
      }
      return seen.get(key);
    };
    const n = countsOf(RADIX_PASSES[0][0], RADIX_PASSES[0][1], 0).count;
    const f = new DataView(new ArrayBuffer(4));
    return ranksOf(n).map((k) => {
      let prefix = 0;
      for (const [pb, b] of RADIX_PASSES) {
        // `below` holds every key under a smaller prefix: rank k of the region is rank k - below among this pass's bins
        const h = countsOf(pb, b, prefix);
        let j = 0;
        for (let cum = h.counts[0]; cum <= k - h.below; cum += h.counts[++j]);
        prefix = prefix * 2 ** b + j;
      }
      f.setUint32(0, prefix >= 2147483648 ? prefix - 2147483648 : 4294967295 - prefix);
      return f.getFloat32(0);
    });
  }
  /** the exact k-th smallest densities (0-based ranks) of a region, as float32 values: three vx_histogram KEY passes (11, 11
   *  and 10 bits) per rank, the first shared by all ranks.  opts: { source, box } as histogram().  An empty region is refused. */
  densityOrderStatistic(ranks, { source = 'volume', box = null } = {}) {
    const p = this._histogramParams('densityOrderStatistic', source, box);
    checkRanks('densityOrderStatistic', ranks);
    return Float32Array.from(this._orderStatistics(p, (n) => {
      if (n === 0) throw new Error('densityOrderStatistic: the region is empty');
      return checkRanks('densityOrderStatistic', ranks, n);
    }));
  }
  /** the q-th percentile(s) of the densities of a region, exact: the order statistic of rank floor(q / 100 * (n - 1)), NumPy's
   *  method 'lower'.  q: a number (returns a number) or a sequence of numbers (returns a Float32Array) in [0, 100]. */
  densityPercentile(q, { source = 'volume', box = null } = {}) {
    const [qs, scalar] = checkPercentiles('densityPercentile', q);
    const p = this._histogramParams('densityPercentile', source, box);
    const v = this._orderStatistics(p, (n) => {
      if (n === 0) throw new Error('densityPercentile: the region is empty');
      return qs.map(a => Math.floor(a / 100 * (n - 1)));
    });
    return scalar ? v[0] : Float32Array.from(v);
  }
  /** Otsu's threshold of a region from one histogram(opts): the upper edge of the bin that maximises the between-class
   *  variance, so that threshold(t) is the bright class; voxels below or above the range are ignored; fewer than two non-empty
   *  bins are refused */
  otsuThreshold(opts = {}) {
    const h = this.histogram(opts);
    const k = otsuSplit(h.counts, h.edges);
    if (k < 0) throw new Error(`otsuThreshold: fewer than two non-empty bins among the ${h.counts.length}: nothing to split`);
    return h.edges[k + 1];
  }
  /** the last histogram pass: kernels launched and the times of the histogram and of the moments' reduction */
  histogramStats() { return nativeHistogram.histogramStats(this.ctx); }
  /** vx_segment_write_mask, the inverse of segmentMask(): installs a Uint8Array of X*Y*Z/8 bytes (one bit per voxel of
   *  (z, y, x) in C order, LSB first) as the current segment -> what segment() returns, for that mask */
  setSegmentMask(bits) {
    const e = this.sliceExtent();
    if (!(bits instanceof Uint8Array) || bits.length !== e[0] * e[1] * e[2] / 8)
      throw new Error(`setSegmentMask: bits must be a Uint8Array of ${e[0] * e[1] * e[2] / 8} bytes`);
    this.bindUniforms();
    return this._segmentResult(native.setSegmentMask(this.ctx, bits));
  }
  _segmentResult(r) {
    r.mean = r.count ? r.dSum / r.count : NaN;
    if (this.segmentView !== 'off') this.restartRendering();   // the masked views show the new mask
    return r;
  }
  /** the last segmentEdit or setSegmentMask: kernels launched and the times of the edit and of the statistics */
  segmentEditStats() { return native.segmentEditStats(this.ctx); }
  /** vx_segment_threshold: the whole band lo <= d <= hi (inside box) as the current segment, without a seed; opts: { hi =
   *  Infinity, box = null } -> what segment() returns (rounds = brickVisits = 0).  Binds the current uniforms first. */
  threshold(lo, { hi = Infinity, box = null } = {}) {
    const e = this.sliceExtent();
    const [l32, h32] = checkBand('threshold', lo, hi), [blo, bhi] = checkBox('threshold', box, e);
    const p = new ParamsBlock(SEGMENT_LAYOUT);
    p.set('seed', [0, 0, 0]); p.set('lo', l32); p.set('hi', h32); p.set('connectivity', 6);
    p.set('box_lo', blo); p.set('box_hi', bhi); p.set('max_rounds', 0);
    this.bindUniforms();
    return this._segmentResult(native.segmentThreshold(this.ctx, p.buffer));
  }
  _islandsCall(name, op, connectivity, keep = 0, minVoxels = 0, seed = [0, 0, 0]) {
    checkConnectivity(name, connectivity);
    this.bindUniforms();
    const r = native.segmentIslands(this.ctx, op, connectivity, keep, minVoxels, seed[0], seed[1], seed[2]);
    this._islandRows = r.kept;
    r.seg.mean = r.seg.count ? r.seg.dSum / r.seg.count : NaN;
    if (op !== 0 && this.segmentView !== 'off') this.restartRendering();   // the masked views show the new mask
    return r;
  }
  /** vx_segment_islands, LABEL (DESIGN.md section 2 "Islands"): the 6- / 26-connected components of the current segment, by
   *  voxel count descending, ties by the first voxel in C order -> { count, largest, sizes: Float64Array, table: [{ label, count,
   *  anchor, bboxLo, bboxHi }], segment, labels(): Uint32Array over (z, y, x) }.  The segment is not changed. */
  islands({ connectivity = 6 } = {}) {
    const r = this._islandsCall('islands', 0, connectivity);
    const table = native.islandsRead(this.ctx, 0, r.kept);
    return { count: r.islands, largest: r.largest, sizes: Float64Array.from(table, t => t.count), table, segment: r.seg,
             labels: () => this.islandLabels() };
  }
  /** the dense label volume of the current island table (vx_islands_read_labels) */
  islandLabels() {
    const e = this.sliceExtent();
    const out = new Uint32Array(e[0] * e[1] * e[2]);
    native.islandsReadLabels(this.ctx, out);
    return out;
  }
  _islandSegment(r) { return Object.assign(r.seg, { islands: r.islands, kept: r.kept, largest: r.largest }); }
  /** keeps the n largest islands of the current segment -> what segment() returns for the new mask, with islands (before),
   *  kept (after) and largest */
  keepLargestIslands(n = 1, { connectivity = 6 } = {}) {
    if (!Number.isInteger(n) || n < 1) throw new Error(`keepLargestIslands: n must be an integer >= 1, not ${n}`);
    return this._islandSegment(this._islandsCall('keepLargestIslands', 1, connectivity, n));
  }
  /** removes the islands of fewer than minVoxels voxels from the current segment */
  removeSmallIslands(minVoxels, { connectivity = 6 } = {}) {
    if (!Number.isInteger(minVoxels) || minVoxels < 1) throw new Error(`removeSmallIslands: minVoxels must be an integer >= 1, not ${minVoxels}`);
    return this._islandSegment(this._islandsCall('removeSmallIslands', 2, connectivity, 0, minVoxels));
  }
  /** keeps the island of the current segment that holds voxel = [x, y, z] (the empty set when the voxel is not in it) */
  keepIslandAt(voxel, { connectivity = 6 } = {}) {
    checkVoxel('keepIslandAt', 'voxel', voxel, this.sliceExtent());
    return this._islandSegment(this._islandsCall('keepIslandAt', 3, connectivity, 0, 0, voxel));
  }
  /** the last islands call: kernels launched and the times of its passes; hostRankMs is the host's ranking of the rows */
  islandsStats() { return native.islandsStats(this.ctx); }
  /** vx_mesh_extract (DESIGN.md section 2 "Meshes"): the surface of the isosurface d = iso, or ({ segment: true }) of the current
   *  segment, as a closed indexed triangle mesh built on the GPU (naive surface nets).  opts: { iso | segment, box = null
   *  ([[x0, y0, z0], [x1, y1, z1]], inclusive; voxels outside count as outside: the mesh is capped there), space = 'world'
   *  ('voxel': voxel i at i; 'grid': grid.transform * (q + 1/2); 'world': the space of pick()), maxVertices = 0, maxTriangles
   *  = 0 (0: 2^32 - 2) } -> { vertices: Float64Array (3 per vertex), cells: Int32Array (3 per vertex), triangles: Uint32Array
   *  (3 per triangle, normals pointing out) }.  Binds the current uniforms first. */
  extractMesh({ iso = null, segment = false, box = null, space = 'world', maxVertices = 0, maxTriangles = 0 } = {}) {
    if (typeof segment !== 'boolean') throw new Error(`extractMesh: segment must be a boolean, not ${segment}`);
    if ((iso === null) === !segment) throw new Error('extractMesh takes exactly one of iso and segment: true');
    if (!MESH_SPACES.includes(space)) throw new Error(`extractMesh: space must be one of ${MESH_SPACES.join(', ')}, not ${space}`);
    for (const [k, v] of [['maxVertices', maxVertices], ['maxTriangles', maxTriangles]])
      if (!Number.isInteger(v) || v < 0 || v > 4294967295) throw new Error(`extractMesh: ${k} must be an integer 0 .. 2^32 - 1, not ${v}`);
    const i32 = segment ? 0 : Math.fround(iso);
    if (!segment && !(Number.isFinite(i32) && i32 > 0)) throw new Error(`extractMesh: iso must be finite and > 0, not ${iso}`);
    const [blo, bhi] = checkBox('extractMesh', box, this.sliceExtent());
    const p = new ParamsBlock(MESH_LAYOUT);
    p.set('source', segment ? 1 : 0); p.set('iso', i32); p.set('box_lo', blo); p.set('box_hi', bhi);
    p.set('max_vertices', maxVertices); p.set('max_triangles', maxTriangles);
    this.bindUniforms();
    const res = native.meshExtract(this.ctx, p.buffer);
    const v32 = new Float32Array(3 * res.vertices), cells = new Int32Array(3 * res.vertices);
    let triangles = new Uint32Array(3 * res.triangles);
    native.meshRead(this.ctx, v32, cells, triangles);
    const vertices = Float64Array.from(v32);
    if (space !== 'voxel') {
      // m * (q + 1/2, 1) in doubles; voxel i occupies [i, i + 1] in index space
      const m = Array.from(space === 'grid' ? this.volume.grid.transform : this.densityTransform());
      for (let k = 0; k < vertices.length; k += 3) {
        const x = vertices[k] + 0.5, y = vertices[k + 1] + 0.5, z = vertices[k + 2] + 0.5;
        for (let r = 0; r < 3; ++r) vertices[k + r] = m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r];
      }
      const det = m[0] * (m[5] * m[10] - m[9] * m[6]) - m[4] * (m[1] * m[10] - m[9] * m[2]) + m[8] * (m[1] * m[6] - m[5] * m[2]);
      if (det < 0) for (let k = 0; k < triangles.length; k += 3) { const t = triangles[k + 1]; triangles[k + 1] = triangles[k + 2]; triangles[k + 2] = t; }
    }
    return { vertices, cells, triangles };
  }
  /** the last extractMesh: kernels launched (the same for every mesh) and the times of its three stages (vx_mesh_stats) */
  meshStats() { return native.meshStats(this.ctx); }
  /** binary STL of a mesh from extractMesh: an 80-byte header, the u32 triangle count, 50 bytes per triangle (the unit facet
   *  normal of the float32 corners, (0, 0, 0) for a degenerate one) -- the bytes of Mesh.write_stl in Python */
  meshToStl({ vertices, triangles }) {
    const n = triangles.length / 3;
    const out = Buffer.alloc(84 + 50 * n);
    out.fill(' ', 0, 80);
    out.write('volxel_amd binary STL', 0, 'ascii');
    out.writeUInt32LE(n, 80);
    const c = [[0, 0, 0], [0, 0, 0], [0, 0, 0]];
    for (let t = 0; t < n; ++t) {
      for (let k = 0; k < 3; ++k) for (let a = 0; a < 3; ++a) c[k][a] = Math.fround(vertices[3 * triangles[3 * t + k] + a]);
      const u = [c[1][0] - c[0][0], c[1][1] - c[0][1], c[1][2] - c[0][2]], w = [c[2][0] - c[0][0], c[2][1] - c[0][1], c[2][2] - c[0][2]];
      let nx = u[1] * w[2] - u[2] * w[1], ny = u[2] * w[0] - u[0] * w[2], nz = u[0] * w[1] - u[1] * w[0];
      const len = Math.sqrt(nx * nx + ny * ny + nz * nz);
      if (len > 0) { nx /= len; ny /= len; nz /= len; } else { nx = ny = nz = 0; }
      let o = 84 + 50 * t;
      for (const f of [nx, ny, nz, ...c[0], ...c[1], ...c[2]]) { out.writeFloatLE(f, o); o += 4; }
    }
    return out;
  }
  /** 'off' (the default, and again after a new volume), 'only' (the current segment alone) or 'hide' (everything but it):
   *  DVR, Phong, MIP / MinIP and the isosurfaces (hence pick) sample a volume whose hidden voxels read 0 (vx_set_segment_view,
   *  DESIGN.md section 2 "Segment views"); slices and segment() keep the unmasked data.  Setting it restarts accumulation. */
  get segmentView() { return SEGMENT_VIEWS[native.getSegmentView(this.ctx)]; }
  set segmentView(view) {
    const i = SEGMENT_VIEWS.indexOf(view);
    if (i < 0) throw new Error(`segmentView must be one of ${SEGMENT_VIEWS.join(', ')}, not ${view}`);
    native.setSegmentView(this.ctx, i);
    this.restartRendering();
  }
  /** the current segment, one bit per voxel of (z, y, x) in C order, LSB first: a Uint8Array of X*Y*Z/8 bytes */
  segmentMask() {
    const e = this.sliceExtent();
    const bits = new Uint8Array(e[0] * e[1] * e[2] / 8);
    native.segmentMask(this.ctx, bits);
    return bits;
  }
  /** the current segment on a slice spec (axial / coronal / sagittal or { origin, du, dv, dn, size, slabSamples }):
   *  { mask: Uint8Array (W*H, 0 / 1, row 0 = y = 0), width, height } */
  sliceMask({ origin, du, dv, dn, size, slabSamples = 1 }) {
    const p = sliceParams('sliceMask', origin, du, dv, dn, size, slabSamples), [W, H] = size;
    const mask = new Uint8Array(W * H);
    native.sliceMask(this.ctx, p.buffer, mask);
    return { mask, width: W, height: H };
  }
  /** the voxel [x, y, z] nearest a world point, or null outside the volume: q = density_transform_inv * w - 1/2 in doubles,
   *  with the float32 matrix the uniforms carry (densityTransformInv, as bindUniforms sends it), each row summed x, y, z,
   *  translation in that order, then floor(q + 1/2) per axis -- what Renderer.voxel_index does in Python */
  voxelIndex(w) {
    if (!this.volume) throw new Error('voxelIndex: no volume');
    if (!(Array.isArray(w) && w.length === 3 && w.every(Number.isFinite))) throw new Error('voxelIndex: w must be three finite numbers');
    const e = this.volume.grid.indexExtent;
    const m = this.densityTransformInv().map(Math.fround);
    const q = [0, 1, 2].map(r => m[r] * w[0] + m[4 + r] * w[1] + m[8 + r] * w[2] + m[12 + r] - 0.5);
    const i = q.map(a => Math.floor(a + 0.5));
    return i.every((x, a) => x >= 0 && x < e[a]) ? i : null;
  }
  /** the last segment: rounds, brickVisits and the times of its predicate pass, flood and statistics (vx_segment_stats) */
  segmentStats() { return native.segmentStats(this.ctx); }
}

function sliceSpec(name, i, n, origin, du, dv, dn, size) {
  if (!Number.isInteger(i) || i < 0 || i >= n) throw new Error(`${name} must be a voxel index in [0, ${n}), not ${i}`);
  return { origin, du, dv, dn, size, slabSamples: 1 };
}

module.exports = { Volxel3DDicomRenderer, Environment, VolxelRenderMode: RenderMode, generateTransferFunction, Camera, native,
  registerVolxelComponents, readZipSlices, decodeEnvironment, fetchBytes, getWorkerFactory: () => workerFactory };
