// Typings of the headless host (names follow volxel-3d-viewer/src/viewer.ts, utils/data.ts, common.ts)
export type ColorStop = { color: [number, number, number, number]; stop: number };
export type BrickGridMessage = {            // WasmWorkerMessageDicomReturn, common.ts:37-55
  type: "return_dicom";
  indirectionSize: [number, number, number]; rangeSize: [number, number, number]; atlasSize: [number, number, number];
  transform: Float32Array; histogram: Uint32Array; histogramGradientRange: [number, number];
  histogramGradient: Int32Array; minMaj: [number, number]; indexExtent: [number, number, number];
  rangeMipmaps: { mipmap: Uint16Array; stride: [number, number, number] }[];
  indirection: Uint32Array; range: Uint16Array; atlas: Uint8Array; brickCounter: number;
};
/** a plane in the cell frame (q = index position - 1/2): sample s of pixel (x, y) at origin + x*du + y*dv + s*dn */
export type SliceSpec = {
  origin: [number, number, number]; du: [number, number, number]; dv: [number, number, number]; dn: [number, number, number];
  size: [number, number]; slabSamples?: number;
};
export declare const VolxelRenderMode: { default: 0; no_dda: 1; raymarch: 2; dvr: 3; dvr_phong: 4; mip: 5; minip: 6 };
export declare function generateTransferFunction(colors: ColorStop[], generatedSteps?: number): { data: Float32Array; length: number };
/** the region of a histogram call: source 'volume' (default: every voxel), 'segment' (the current segment) or a slot 0 .. 31 of the
 *  segment store; box = [[x0, y0, z0], [x1, y1, z1]], inclusive voxel indices, null (default): the whole index extent */
export type HistogramOptions = { source?: 'volume' | 'segment' | number; box?: [[number, number, number], [number, number, number]] | null };
export declare class Camera {
  pos: number[]; view: number[];
  /** [build] null: the reference's perspective camera (scene.ts:65-72); a number: orthographic, image spans +-orthoHalfHeight world units vertically */
  orthoHalfHeight: number | null;
  yaw: number; pitch: number;
  constructor(distance?: number); viewMatrix(): number[]; projMatrix(aspect: number, fov?: number): number[];
  /** scene.ts:15-52 */
  rotateAroundView(by: [number, number]): void; zoom(by: number): boolean;
  translateOnPlane(by: [number, number]): void; translate(by: [number, number, number]): void;
}
export declare class Environment {          // representation/environment.ts; row 0 of `floats` = top
  constructor(floats: Float32Array, width: number, height: number, strength?: number);
  floats: Float32Array; width: number; height: number; strength: number;
  static default(): Environment;
}
export declare class Volxel3DDicomRenderer {
  /** layout: 0 reference textures, 1 cellquad, 2 brickf32, 3 (default) per render mode, 4 bricku8 (8-bit bricks decoded at staging) -- include/volxel_hip.h VxLayout.
   *  device: one GPU (HIP ordinal, default 0).  devices: one image on several GPUs (member i renders shard i, an id
   *  may repeat); excludes device. */
  constructor(opts?: { width?: number; height?: number; device?: number; devices?: number[]; layout?: number; lowResPreview?: boolean });
  readonly devices: number[] | null;
  environment: Environment | null;
  setEnvironment(env: Environment | null): void;
  settings: Record<string, any>; camera: Camera; envStrength: number; frameIndex: number;
  renderMode: keyof typeof VolxelRenderMode;
  restartFromFiles(files: (string | Uint8Array)[], threads?: number): void;
  /** viewer.ts:977-1040.  ZIP (stored / deflate) and Radiance RGBE are decoded by the host; URLs are paths or file:// URLs
   *  (no fetch in this Node); OpenEXR bytes are refused with a message naming setupEnv(). */
  restartFromZip(zip: string | Uint8Array, threads?: number): void;
  restartFromZipUrl(url: string, threads?: number): void;
  restartFromURLs(urls: string[], threads?: number): void;
  loadEnv(bytes: Uint8Array): void;
  loadEnvFromUrl(url: string): void;
  /** viewer.ts:443-449,543-551,789-795: the light follows the camera when settings.syncLightDir is on */
  maybeSyncLight(): void;
  rotateCamera(by: [number, number]): void;
  syncLightDir: boolean;
  setupEnv(env: { width: number; height: number; floats: Float32Array }): void;
  /** restartFromFiles for slices already read into memory */
  restartFromBytes(files: Uint8Array[], threads?: number): void;
  restartFromVoxels(voxels: Uint16Array, dims: [number, number, number], spacing?: [number, number, number], maxValue?: number, threads?: number): void;
  setupFromGrid(grid: BrickGridMessage): void;
  changeTransferFunc(data: Float32Array, length: number): void;
  restartRendering(): void;
  restoreSettings(settings: any): void;
  /** data-benchmark-url runner (viewer.ts:856-890); returns VolxelBenchmarkResult records */
  startBenchmark(collection: { sharedSettings: any[]; benchmarks: any[] }, volumes?: Record<string, BrickGridMessage>): any[];
  bindUniforms(): { buffer: ArrayBuffer };
  render(frames?: number, inFlight?: number): void;
  probeTileCosts(): Uint32Array;
  setTileOrder(perm: Uint32Array | null): void;
  deviceInfo(): { name: string; computeUnits: number; hbmBytes: number };
  finish(): void;
  readAccum(): Float32Array;
  readDisplay(): Uint8Array;
  counters(): { samples: number; rays: number; pixels: number; skipSteps: number; gradSamples: number; tfSamples: number; activeLaneSlots: number; laneSlots: number; launches: number; frames: number;
                kernelMs: number; lastKernelMs: number; gathers: number; ldsReads: number; mergeMs: number; minLaunchFrames: number; maxLaunchFrames: number;
                mergeLaunches: number };
  resetCounters(): void;
  /** shadowed DVR (settings.dvrShadowStride = 1, 2 or 4; include/volxel_hip.h vx_shadow_stats): light-grid builds since
   *  creation, light-march samples and HIP-event time of the last build */
  shadowStats(): { builds: number; lightSamples: number; lastBuildMs: number };
  /** the last light grid built (vx_debug_read_shadow_grid): transmittance toward the light per node, x fastest */
  readShadowGrid(): { dims: [number, number, number]; data: Float32Array };
  /** index-space planes z = k, y = j, x = i through voxel centres, one pixel per voxel (patient orientation not modelled) */
  axial(k: number): SliceSpec;
  coronal(j: number): SliceSpec;
  sagittal(i: number): SliceSpec;
  /** a slice or thick slab on the GPU (include/volxel_hip.h vx_slice): values row-major, row 0 = y = 0; rgba8 with a display */
  slice(spec: SliceSpec & { reduce?: "mean" | "max" | "min"; display?: "grey" | "tf" | null; window?: [number, number] | null }):
    { values: Float32Array; rgba8: Uint8Array | null };
  /** the last slice: W*H*N samples and its HIP-event kernel time */
  sliceStats(): { samples: number; lastKernelMs: number };
  /** the shaded first-hit isosurface of density iso on the GPU (include/volxel_hip.h vx_isosurface): 4 floats per window pixel,
   *  row 0 = y0; hit = (world x, y, z, t), (0, 0, 0, -1) on a miss.  window = [x0, y0, x1, y1] of the render size (GL rows) */
  isosurface(iso: number, opts?: { color?: [number, number, number]; phong?: [number, number, number, number]; refine?: number;
    skip?: boolean; window?: [number, number, number, number] | null }):
    { rgba: Float32Array; hit: Float32Array; width: number; height: number };
  /** the world point under pixel (x, y) (GL rows) on the isosurface iso, or null when the ray misses it */
  pick(x: number, y: number, iso: number, opts?: { refine?: number }): [number, number, number] | null;
  /** the last isosurface: rays, hits, march samples, bisection samples, samples passed over and its HIP-event kernel time */
  isoStats(): { rays: number; hits: number; samples: number; refineSamples: number; skipped: number; lastKernelMs: number };
  /** the connected component of lo <= d <= hi holding voxel seed on the GPU (include/volxel_hip.h vx_segment) */
  segment(seed: [number, number, number], lo: number, opts?: { hi?: number; connectivity?: 6 | 26;
    box?: [[number, number, number], [number, number, number]] | null; maxRounds?: number }):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** the current segment: one bit per voxel of (z, y, x) in C order, LSB first */
  segmentMask(): Uint8Array;
  /** dilate, erode, open, close or fill the holes of the current segment on the GPU (include/volxel_hip.h vx_segment_edit) */
  segmentEdit(op: 'dilate' | 'erode' | 'open' | 'close' | 'fill_holes', opts?: { steps?: number; connectivity?: 6 | 26; band?: boolean }):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** grow, shrink, open or close the current segment by a radius in physical units (include/volxel_hip.h vx_segment_margin) */
  segmentMargin(op: 'grow' | 'shrink' | 'open' | 'close', radius: number,
    opts?: { spacing?: [number, number, number] | null; band?: boolean }):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** the exact Euclidean distance field of the current segment under the voxel spacing (vx_segment_distance); squared() and
   *  distance() read the field over (z, y, x), Infinity beyond maxDistance */
  segmentDistance(opts?: { side?: 'outside' | 'inside'; maxDistance?: number; spacing?: [number, number, number] | null }):
    { finite: number; maxD2: number; maxDistance: number; argmax: [number, number, number]; squared(): Float32Array;
      distance(): Float32Array };
  /** the squared distances of the last segmentDistance over (z, y, x) (vx_distance_read) */
  distanceField(): Float32Array;
  /** the last segmentDistance or segmentMargin: kernels launched and the times of its passes */
  distanceStats(): { launches: number; xMs: number; yMs: number; zMs: number; compareMs: number };
  /** copy the current segment into a slot (0 .. 31) of the device's segment store (include/volxel_hip.h vx_segment_store) */
  storeSegment(slot: number): void;
  /** the mask of a slot becomes the current segment; the slot keeps its copy (vx_segment_load) */
  loadSegment(slot: number):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** free a slot; an empty one is fine (vx_segment_drop) */
  dropSegment(slot: number): void;
  /** the occupied slots, ascending (vx_segment_slots) */
  storedSegments(): number[];
  /** a set operation on the current segment A and the mask B of a slot, in place; 'invert' takes no slot (vx_segment_combine) */
  segmentCombine(op: 'union' | 'intersect' | 'subtract' | 'xor' | 'invert', slot?: number | null):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** overlap counts, Dice, Jaccard and (hausdorff, the default) the directed Hausdorff distances of the current segment A and
   *  the mask B of a slot; the distance fields are null without hausdorff (vx_segment_compare) */
  segmentCompare(slot: number, opts?: { hausdorff?: boolean; spacing?: [number, number, number] | null }):
    { countA: number; countB: number; countAnd: number; dice: number; jaccard: number; d2Ab: number | null; d2Ba: number | null;
      hausdorffAb: number | null; hausdorffBa: number | null; hausdorff: number | null;
      argmaxAb: [number, number, number] | null; argmaxBa: [number, number, number] | null };
  /** the uint8 label map over (z, y, x) of the listed slots, first listed first, and the number of voxels more than one of
   *  them holds (vx_segments_labelmap) */
  segmentsLabelmap(slots: number[] | Uint32Array): { labels: Uint8Array; overlaps: number };
  /** the density histogram and the moments of a region on the GPU (vx_histogram): `bins` (1 .. 4096) bins of equal width over
   *  range = [lo, hi] (default [0, 1]; a density equal to hi lands in the last bin); source 'volume' (default), 'segment' or a
   *  slot of the segment store; box inclusive, null: the whole index extent.  edges are nominal (lo + k (hi - lo) / bins); below /
   *  above count the voxels outside the range; the moments run over the whole region; mean and std (population) are NaN when it
   *  is empty.  Changes nothing. */
  histogram(opts?: HistogramOptions & { bins?: number; range?: [number, number] }):
    { counts: Float64Array; edges: Float64Array; below: number; above: number; count: number; dMin: number; dMax: number;
      dSum: number; dSum2: number; mean: number; std: number };
  /** the exact k-th smallest densities of a region (0-based ranks), the bits a sort would give: a radix select in three
   *  histogram passes per rank, the first shared by all ranks; an empty region is refused */
  densityOrderStatistic(ranks: number[] | Uint32Array, opts?: HistogramOptions): Float32Array;
  /** the exact q-th percentile(s), q in [0, 100]: the order statistic of rank floor(q / 100 * (n - 1)) (NumPy's method 'lower');
   *  a number for a number, a Float32Array for a sequence */
  densityPercentile(q: number, opts?: HistogramOptions): number;
  densityPercentile(q: number[] | Float64Array, opts?: HistogramOptions): Float32Array;
  /** Otsu's threshold from one histogram(opts): the upper edge of the bin that maximises the between-class variance, so that
   *  threshold(t) is the bright class; fewer than two non-empty bins are refused */
  otsuThreshold(opts?: HistogramOptions & { bins?: number; range?: [number, number] }): number;
  /** the last histogram pass: kernels launched and the times of the histogram and of the moments' reduction */
  histogramStats(): { launches: number; histogramMs: number; momentsMs: number };
  /** install a packed mask (the layout of segmentMask()) as the current segment (vx_segment_write_mask) */
  setSegmentMask(bits: Uint8Array):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** the last segmentEdit or setSegmentMask: kernels launched, the times of the edit and of its statistics */
  segmentEditStats(): { launches: number; editMs: number; statsMs: number };
  /** the whole band lo <= d <= hi as the current segment, without a seed (include/volxel_hip.h vx_segment_threshold) */
  threshold(lo: number, opts?: { hi?: number; box?: [[number, number, number], [number, number, number]] | null }):
    { count: number; bboxLo: [number, number, number]; bboxHi: [number, number, number]; dMin: number; dMax: number; dSum: number;
      mean: number; rounds: number; converged: boolean; brickVisits: number };
  /** the islands (connected components) of the current segment, largest first (include/volxel_hip.h vx_segment_islands) */
  islands(opts?: { connectivity?: 6 | 26 }): { count: number; largest: number; sizes: Float64Array;
    table: { label: number; count: number; anchor: [number, number, number]; bboxLo: [number, number, number];
             bboxHi: [number, number, number] }[];
    segment: { count: number; dSum: number; mean: number }; labels(): Uint32Array };
  /** the dense label volume over (z, y, x) of the current island table: 0 outside the segment, k + 1 on island k */
  islandLabels(): Uint32Array;
  /** keep the n largest islands / drop the islands below minVoxels / keep the island under a voxel: the statistics of the new
   *  mask as segment() returns them, with the islands before the op, those kept and the size of the largest */
  keepLargestIslands(n?: number, opts?: { connectivity?: 6 | 26 }): { count: number; islands: number; kept: number; largest: number;
    dSum: number; mean: number; bboxLo: [number, number, number]; bboxHi: [number, number, number] };
  removeSmallIslands(minVoxels: number, opts?: { connectivity?: 6 | 26 }): { count: number; islands: number; kept: number;
    largest: number; dSum: number; mean: number; bboxLo: [number, number, number]; bboxHi: [number, number, number] };
  keepIslandAt(voxel: [number, number, number], opts?: { connectivity?: 6 | 26 }): { count: number; islands: number; kept: number;
    largest: number; dSum: number; mean: number; bboxLo: [number, number, number]; bboxHi: [number, number, number] };
  /** the last islands call: kernels launched and the times of its passes (hostRankMs: the host's ranking of the table) */
  islandsStats(): { launches: number; localMs: number; mergeMs: number; flattenMs: number; tableMs: number; hostRankMs: number;
    applyMs: number; statsMs: number };
  /** the surface of the isosurface d = iso, or of the current segment, as a closed indexed triangle mesh built on the GPU
   *  (include/volxel_hip.h vx_mesh_extract): 3 numbers per vertex, 3 cell components per vertex, 3 indices per triangle */
  extractMesh(opts: { iso?: number; segment?: boolean; box?: [[number, number, number], [number, number, number]] | null;
    space?: 'voxel' | 'grid' | 'world'; maxVertices?: number; maxTriangles?: number }):
    { vertices: Float64Array; cells: Int32Array; triangles: Uint32Array };
  /** the last extractMesh: kernels launched and the times of the inside words, the active cells with their scan, the emission */
  meshStats(): { launches: number; insideMs: number; activeMs: number; emitMs: number };
  /** binary STL (80-byte header, u32 count, 50 bytes per triangle) of a mesh from extractMesh */
  meshToStl(mesh: { vertices: Float64Array; triangles: Uint32Array }): Buffer;
  /** show only, or hide, the current segment in DVR, Phong, MIP / MinIP and the isosurfaces (vx_set_segment_view); 'off' after
   *  a new volume; setting it restarts accumulation */
  segmentView: 'off' | 'only' | 'hide';
  /** the current segment on a slice spec: 0 / 1 per pixel, row 0 = y = 0 */
  sliceMask(spec: { origin: number[]; du: number[]; dv: number[]; dn: number[]; size: [number, number]; slabSamples?: number }):
    { mask: Uint8Array; width: number; height: number };
  /** the voxel nearest a world point, or null outside the volume */
  voxelIndex(w: [number, number, number]): [number, number, number] | null;
  /** the last segment: flood rounds, brick visits and the times of its predicate pass, flood and statistics */
  segmentStats(): { rounds: number; brickVisits: number; predicateMs: number; floodMs: number; statsMs: number };
  dispose(): void;
}
/** viewer.ts:1455-1462: keeps the worker factory, returns the element-name -> class table ("volxel-3d-viewer") */
export declare function registerVolxelComponents(worker?: () => unknown): Record<string, typeof Volxel3DDicomRenderer>;
export declare function readZipSlices(zip: Uint8Array): Uint8Array[];
export declare function decodeEnvironment(bytes: Uint8Array): { floats: Float32Array; width: number; height: number };
