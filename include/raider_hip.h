/* raider_hip.h - C ABI of libraider_hip.so, the MI355X (gfx950) engine behind RAiDER's delay hot path.
 *
 * Drop-in boundary: these are the entry points a RAiDER maintainer's ctypes binding would call in
 * place of the reference's NumPy/scipy/pyproj hot loops and its two native extensions.  Every entry
 * cites the reference interface it replaces (paths relative to the RAiDER repository root).
 * INTEGRATION.md shows the reference-side ctypes stub.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  Every function returns an int status
 *     (RDR_OK or a negative RDR_ERR_*); rdr_last_error() gives the message.
 *   - the caller owns every buffer it passes; the library owns device memory behind the opaque
 *     rdr_ctx / rdr_cube handles and never returns an allocation.
 *   - `loc` says where the caller's arrays live: RDR_HOST (NumPy) - the library stages them through
 *     its own device scratch and copies results back; RDR_DEVICE - pointers are HIP device pointers
 *     (e.g. torch tensors), kernels are launched on the ctx stream and NOT synchronised.
 *   - all floating point arrays are float64 unless a dtype argument says otherwise; angles in degrees,
 *     lengths in metres; NaN is the in-band missing value exactly as in the reference.
 *   - one ctx = one device + one stream; a ctx is not thread-safe, distinct ctxs are.
 *   - argument errors never reach the device: a NULL pointer where an array is needed, a negative count, an unknown mode /
 *     dtype / direction is RDR_ERR_INVALID with the reason in rdr_last_error; a count of 0 is an empty batch (RDR_OK, nothing
 *     touched).  A HIP failure the library reports (RDR_ERR_HIP, e.g. out of memory) leaves no error state behind: the
 *     next call starts clean.  rdr_last_error(ctx) is the context's last message, rdr_last_error(NULL) the calling thread's.
 */
#ifndef RAIDER_HIP_H
#define RAIDER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDR_OK 0
#define RDR_ERR_INVALID (-1)    /* bad argument                -> TypeError / ValueError in the shim       */
#define RDR_ERR_HIP (-2)        /* HIP runtime failure         -> RuntimeError                             */
#define RDR_ERR_NODEVICE (-3)   /* no usable GPU               -> RuntimeError (product never falls back)  */
#define RDR_ERR_ALL_NAN (-4)    /* every ray length is NaN     -> ValueError('geo2rdr did not converge...') delay.py:279-280 */
#define RDR_ERR_NO_LEVELS (-5)  /* no model interval contributes: build_ray returns (None,None,None) losreader.py:832-833 */
#define RDR_ERR_NAN_LENGTH (-6) /* some (not all) ray lengths NaN: the reference's nParts (delay.py:283) is undefined there */
#define RDR_ERR_OOM (-7)        /* the device could not hold an allocation (hipErrorOutOfMemory) -> MemoryError; the caller may retry with a smaller batch */

#define RDR_F32 0
#define RDR_F64 1
#define RDR_I16 2 /* int16 elements: rasters only (rdr_raster_sample / rdr_raster_bounds; a DEM in its file type) */
#define RDR_BYTESWAPPED 0x100 /* or-ed into the dtype of rdr_cube_create: the source fields are in the OTHER byte order than the host
                               * (a NetCDF-3 file is big-endian) - swapped on the device while packing, so a file mapping is uploaded as is */
#define RDR_HOST 0
#define RDR_DEVICE 1

/* ray origin modes */
#define RDR_ORIGIN_GRID 0 /* meshgrid(xpts, ypts) at height ht, row-major (ny,nx)  delay.py:242,262-267 */
#define RDR_ORIGIN_LLH 1  /* per-ray lat[n], lon[n] at height ht                                   */
#define RDR_ORIGIN_XYZ 2  /* per-ray ECEF xyz[n,3] (already at height ht)                          */
/* look-vector modes */
#define RDR_LOS_VEC 0      /* los[n,3] unit ECEF, ground->sensor: what los.getLookVectors returns, delay.py:270 */
#define RDR_LOS_INC_HD 1   /* inc[n], hd[n] degrees -> inc_hd_to_enu + enu2ecef  losreader.py:374-396, utilFcns.py:91-121 */
#define RDR_LOS_INC_HD_SCALAR 2 /* one inc0/hd0 for every ray                                       */
#define RDR_LOS_ZENITH 3   /* getZenithLookVecs, losreader.py:302-316                               */

/* flag bits returned by rdr_ray_prepass / consumed by rdr_ray_march */
#define RDR_FLAG_ANY_NAN 1        /* some ray length is NaN                                          */
#define RDR_FLAG_ANY_FINITE 2     /* some ray length is finite                                       */
#define RDR_FLAG_FIRST_NOT_BELOW 4 /* some ray's first sample is NOT below min(model_zs)  (delay.py:306) */
#define RDR_FLAG_LAST_NOT_ABOVE 8  /* some ray's last sample is NOT above max(model_zs)   (delay.py:310) */
#define RDR_FLAG_DIVERGED 16      /* a level's maximum ray length asks for more than 65536 integration parts (or is not
                                    * finite): the level crossings diverged, e.g. look vectors far from unit length.  The
                                    * slice's outputs are NaN and synchronous calls return RDR_ERR_INVALID.               */

#define RDR_FLAG_BAD_HEIGHT 32    /* per-ray heights: some rays->hts[i] lies below the `ht` the batch's level table was built for:
                                    * the outputs are NaN and synchronous calls return RDR_ERR_INVALID.                        */

#define RDR_FLAG_NAN_OUTPUT 64    /* rdr_raytrace_slices: some delay of the slice is NaN (what delay.py:187 scans the result for) */

typedef struct rdr_ctx rdr_ctx;
typedef struct rdr_cube rdr_cube;

/* Ray batch = one (ny,nx) slice of _build_cube_ray at one height `ht` (delay.py:256-273). */
typedef struct rdr_rays {
    int64_t n;          /* number of rays (ny*nx in GRID mode)                                  */
    int32_t origin_mode;
    int32_t los_mode;
    int64_t nx, ny;     /* GRID mode                                                            */
    const double* xpts; /* GRID: [nx] lon deg                                                   */
    const double* ypts; /* GRID: [ny] lat deg                                                   */
    const double* lat;  /* LLH: [n]                                                             */
    const double* lon;  /* LLH: [n]                                                             */
    const double* xyz;  /* XYZ: [n,3]; with an inc/heading or zenith LOS lat/lon are needed too */
    const double* los;  /* LOS_VEC: [n,3]                                                       */
    const double* inc;  /* LOS_INC_HD: [n]                                                      */
    const double* hd;   /* LOS_INC_HD: [n], or NULL: heading hd0 for every ray                  */
    double inc0, hd0;   /* LOS_INC_HD_SCALAR (hd0 also: LOS_INC_HD with hd == NULL)             */
    int32_t loc;        /* RDR_HOST / RDR_DEVICE for every pointer above                        */
    int32_t _pad;
    const double* hts;  /* NULL: every ray starts at the `ht` of the call (the reference's slice, delay.py:256-273).
                         * [n]: PER-RAY origin heights (a scene on a DEM; BASELINE configs "c3b").  The reference has no
                         * such batch; the rule is its slice algorithm ray by ray: the level tests of
                         * losreader.py:785-808 with the ray's own height (its first contributing interval gets the
                         * 10-iteration crossings and fixes its cos_factor), nParts[k] from the maximum over the rays level k
                         * contributes to (delay.py:283), the all-pixels z-clamp asked about every ray's own first / last
                         * sample.  Equal heights reproduce the slice result bit for bit.  The `ht` argument of the ray
                         * entry points must then be <= min(hts) - normally min(hts): it fixes the batch's level table
                         * (K, the layout of maxlen / nparts); a ray whose no interval contributes gets 0.
                         * GRID / LLH origins are placed at hts[i]; XYZ origins are taken as given.  Not with
                         * rdr_raytrace_slices.                                                     */
} rdr_rays;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int rdr_version(void);
/* sha256[:16] over the sources the library was compiled from (every .h / .hip under raider_amd/csrc + this header; "unknown" when the
 * build recipe did not pass it).  raider_amd._lib.source_hash() computes the same digest from the tree. */
const char* rdr_source_hash(void);
/* device < 0: use HIP's current device.  Fails with RDR_ERR_NODEVICE when there is no GPU. */
int rdr_create(int device, rdr_ctx** out);
void rdr_destroy(rdr_ctx* ctx);
/* message of the last failure on this thread (ctx may be NULL) */
const char* rdr_last_error(rdr_ctx* ctx);
/* Launch on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).  NULL is HIP's default stream;
 * (void*)-1 goes back to the ctx's private stream.  RDR_DEVICE arrays are only ordered against work on THIS stream. */
int rdr_set_stream(rdr_ctx* ctx, void* hip_stream);
/* Tell the context that a stream handed to rdr_set_stream is about to be destroyed: its pending work is waited for if it is still the
 * current stream (the context then goes back to its private stream) and no event is recorded on it ever again (buffers of destroyed
 * cubes are recycled behind events on the streams that used them).  Streams that live as long as the process (torch's) need no call. */
int rdr_forget_stream(rdr_ctx* ctx, void* hip_stream);
int rdr_synchronize(rdr_ctx* ctx);
int rdr_device_info(rdr_ctx* ctx, char* name, int name_len, int* compute_units, int64_t* total_mem);
/* profiling: while on, a HIP event pair brackets every kernel launch on the ctx stream (no sync).
 * rdr_set_profiling(on) also resets the counters.  rdr_profile_get synchronises on the recorded
 * events and returns how many launches of kernel kind `which` (0 ray prepass, 1 ray march, 2 interp,
 * 3 other) were recorded and their summed duration in ms. */
int rdr_set_profiling(rdr_ctx* ctx, int on);
/* Page-locked host memory for result arrays (hipHostMalloc): downloads into it run at the link rate, without first-touch page
 * faults, and asynchronously - rdr_raytrace_slices overlaps them with the kernels of the next slices.  The Python layer keeps a
 * recycling pool of such blocks behind the delay cubes tropo_delay returns (raider_amd/_pinned.py). */
int rdr_host_alloc(int64_t bytes, void** out);
int rdr_host_free(void* p);
/* Ray pass 1 hands each ray's record to pass 2 through an HBM workspace of 232 B per ray (29 doubles: the degree-5 ray
 * polynomials h(u), lat(u), lon(u), the degree-7 level-crossing polynomial, the ray-length scale and the two crossings of
 * the first level; 3.7 GB for 16 M rays).  The few rays the static classification sends to the generic-geodesy kernels
 * (poles, grazing incidence, the +-180 deg meridian) keep origin / look vector / origin frame in the same record and their
 * K+1 level crossings in a compact side buffer sized for 1/32 of the batch (or for the generic-ray count last seen on this
 * ctx); a generic ray that finds it full has its crossings recomputed by pass 2.
 * `bytes` caps records + side buffer (default 48 GiB of the 288 GB, and never more than half of the free memory); larger
 * batches are integrated in chunks.  Env override at rdr_create: RAIDER_HIP_WORKSPACE_BYTES. */
int rdr_set_workspace_limit(rdr_ctx* ctx, int64_t bytes);
/* Give device memory back: the context keeps its scratch (staging slots, the intermediate cube of rdr_point_delays, the ray-record
 * workspace) and up to 4 GiB of value buffers of destroyed cubes for the next call of the same size.  rdr_trim waits for the
 * context's streams, then frees every scratch buffer larger than `keep_bytes` and pooled buffers until at most `keep_bytes` remain
 * (0: everything); *released (may be NULL) = bytes freed.  rdr_point_delays trims its own intermediates above
 * RAIDER_HIP_SCRATCH_KEEP_BYTES (default 4 GiB) before it returns. */
int rdr_trim(rdr_ctx* ctx, int64_t keep_bytes, int64_t* released);
/* Columns of the generic-ray side buffer: >= 0 fixes the capacity (0: always recompute), -1 restores the automatic sizing. */
int rdr_set_side_capacity(rdr_ctx* ctx, int64_t columns);
int rdr_profile_get(rdr_ctx* ctx, int which, int* count, float* total_ms);
/* diagnostics: the shader clock the chip ACTUALLY runs at while the ctx's kernels execute (it is managed by power: fp64-dense kernels
 * run near 2.0 GHz, not at the data sheet's 2.4).  _begin puts one sleeping wave on the ctx's copy stream for `ms` of wall time; it
 * reads the shader-clock counter and the 100 MHz wall counter before and after.  _end waits for it and returns cycles / wall time
 * in GHz.  Launch the kernels to be observed between the two calls. */
int rdr_clock_sample_begin(rdr_ctx* ctx, double ms);
int rdr_clock_sample_end(rdr_ctx* ctx, double* ghz);
/* diagnostics: resources of the light ray kernel a GRID + look-vector batch on `cube` launches (which 0: pass 1 crossings_kernel,
 * 1: pass 2 march_kernel; 2 / 3: their per-ray-height instantiations, rdr_rays.hts; 4 / 5: the stacked march of
 * rdr_raytrace_slices_epochs for 2 / 4 epochs; 6 / 7: the per-ray-height stacked march of rdr_raytrace_epochs for 2 / 4 epochs), read from the loaded code object (hipFuncGetAttributes): vector registers per lane, static LDS bytes,
 * dynamic LDS bytes of the launch (axis / level tables), scratch bytes per lane, max threads per block.  Any output may be NULL. */
int rdr_ray_kernel_attributes(rdr_ctx* ctx, const rdr_cube* cube, int which, int32_t* vgprs, int32_t* static_lds, int32_t* dynamic_lds,
                              int32_t* scratch, int32_t* max_threads);
/* diagnostics: rays the static classification sent to the generic-geodesy kernels in the last ray pass 1 whose result this ctx read
 * back (rdr_ray_prepass, and rdr_raytrace / rdr_raytrace_slices when they synchronise); -1 for a NULL ctx */
int64_t rdr_generic_ray_count(rdr_ctx* ctx);
/* diagnostics: 64-ray waves of the last rdr_ray_prepass that left the per-level length loop of pass 1 out because their length bounds
 * could not raise any level maximum of the slice (0 with RAIDER_HIP_PASS1_SKIP=0; results never depend on it); -1 for a NULL ctx */
int64_t rdr_skipped_wave_count(rdr_ctx* ctx);
/* diagnostics: rdr_raytrace calls of this ctx that fitted and marched their rays in ONE kernel on a probed partition (one f32 lon/lat cube on
 * exactly uniform axes, one slice of GRID rays with per-pixel look vectors in device arrays, 2 < K <= 128; RAIDER_HIP_ONE_PASS=0: none),
 * and how many of those found the probed partition - or a ray - to need the two classic passes after all, which then ran behind it on the
 * device (as of the last partition this ctx read back: no synchronisation of its own).  Results never depend on the route; -1 for a NULL ctx */
int64_t rdr_one_pass_count(rdr_ctx* ctx);
int64_t rdr_one_pass_redo_count(rdr_ctx* ctx);

/* ---- weather cube ----------------------------------------------------------------------------
 * Replaces getInterpolators (tools/RAiDER/delayFcns.py:23-58): the two fields of one processed weather
 * model (`wet`/`hydro` f32, or `wet_total`/`hydro_total` f64) on a rectilinear (y,x,z) grid, wrapped
 * with scipy-RegularGridInterpolator semantics (linear, bounds_error=False, fill_value=nan).
 * wet/hydro: element [iy,ix,iz] at  base + iy*sy + ix*sx + iz*sz  (ELEMENT strides), so both the
 * file order (z,y,x) (weatherModel.py:685-693) and the transposed (y,x,z) order are accepted without
 * a host-side transpose.  Axes may be ascending or descending (scipy flips; so do we, on device).
 * The device copy interleaves (wet,hydro) per cell, z fastest.  */
int rdr_cube_create(rdr_ctx* ctx, const double* ys, int64_t ny, const double* xs, int64_t nx,
                    const double* zs, int64_t nz, const void* wet, const void* hydro, int dtype,
                    int64_t sy, int64_t sx, int64_t sz, int loc, rdr_cube** out);
void rdr_cube_destroy(rdr_cube* cube);
/* Synchronisation of cube-making entries (round 5).  loc == RDR_HOST: the call returns when the cube is complete (the host arrays may be
 * reused at once).  loc == RDR_DEVICE - cubes made from device arrays, the intermediate delay cubes of rdr_build_cube_to_cube /
 * rdr_raytrace_slices_to_cube - and rdr_cube_blend: NO host synchronisation; the cube is complete in stream order on the context's stream,
 * every entry that reads it from another stream (or another context) first makes that stream wait for the cube's ready event, and the
 * source device arrays must stay valid in stream order, as for any asynchronous kernel.  rdr_set_stream orders the new stream after
 * everything enqueued on the previous one (the context's scratch and flag words are shared by them).
 * Small HOST inputs of any entry (the axes of a cube, AOI axes, height lists; up to 1 MiB each) go up through a ring of page-locked
 * buffers: the caller's array is consumed when the call returns and the host does not wait for work queued earlier on the stream - so the
 * creation of a cube from device arrays, and rdr_build_cube_to_cube / rdr_raytrace_slices_to_cube with host axes, really are asynchronous
 * (round 6; before, the pageable copy of the axes waited for the stream).  Larger host inputs are waited for (one event behind their copy):
 * a host array may be reused as soon as the call that took it returns, whatever memory it lives in.
 * rdr_cube_has_nan: 1 when a NaN was seen among the two source fields while the cube was packed (what delayFcns.py:50-52 scans for on the
 * host: "Weather model contains NaNs!"), 0 otherwise (blended cubes: either source's; a view: its source's), -1 for NULL.  For an
 * asynchronously made cube this call is where the host waits (for that cube's ready event, once). */
int rdr_cube_has_nan(const rdr_cube* cube);
int rdr_cube_shape(const rdr_cube* cube, int64_t* ny, int64_t* nx, int64_t* nz, int* dtype);
/* ascending copies of the axes as the interpolator's `.grid` exposes them (delay.py:239) */
int rdr_cube_axes(const rdr_cube* cube, double* ys, double* xs, double* zs);
/* Projected weather models (HRRR Lambert conformal conic, models/hrrr.py:248-259): tell the cube that its x/y axes are
 * projected metres.  Every entry point that takes GEODETIC query coordinates (rdr_build_cube's xpts/ypts = lon/lat,
 * the ray tracer's samples) then applies geodetic -> model CRS on the device - the pyproj step of delay.py:207-209,253,295.
 * kind RDR_PROJ_LCC, params = {a, es, lat_1, lat_2, lat_0, lon_0, x_0, y_0} (m, -, deg, deg, deg, deg, m, m); es = 0 for
 * HRRR's sphere (a = 6371229).  rdr_interp3 keeps taking points already in cube coordinates (scipy semantics). */
#define RDR_PROJ_LONLAT 0
#define RDR_PROJ_LCC 1
#define RDR_PROJ_STERE 2   /* POLAR stereographic: params = {a, es, lat_0 (+-90), lat_ts (NaN: use k_0), k_0, lon_0, x_0, y_0} (HRRR-AK, models/hrrr.py:22-25) */
int rdr_cube_set_projection(rdr_cube* cube, int kind, const double* params, int nparams);
/* A VIEW of a cube: a second handle on the same device buffers (values, axes, corner-quad copy - nothing is copied or uploaded)
 * that owns only its projection.  The reference builds its pyproj transformers afresh in every call (delay.py:196-216,238-253) and
 * shares nothing between calls; a cube cached per weather-model file and handed to several callers (threads, model CRS arguments)
 * must therefore never be re-projected in place - each call takes a view with the projection IT was given and destroys it afterwards.
 * kind / params as rdr_cube_set_projection; kind -1: the source's own projection.  `ctx` = the context the view is used from (may
 * differ from the source's).  The buffers live until the source AND every view are destroyed, in any order. */
int rdr_cube_view(rdr_ctx* ctx, const rdr_cube* cube, int kind, const double* params, int nparams, rdr_cube** out);
/* transformPoints (delay.py:404-436) for EPSG:4326 -> the cube's CRS: (lat, lon) deg -> (y, x) model coordinates */
int rdr_project_points(rdr_ctx* ctx, const rdr_cube* cube, const double* lat, const double* lon, int64_t n, double* y, double* x, int loc);
/* transformPoints (delay.py:404-436) between EPSG:4326 and a TRANSVERSE-MERCATOR CRS (every UTM zone, EPSG:326xx / 327xx; national
 * TM grids) - the pyproj call behind output grids that are not lon/lat (delay.py:207-209,259-263).  params = {a, es, lat_0, lon_0,
 * k_0, x_0, y_0} (m, -, deg, deg, -, m, m).  direction 0: in = (lat, lon) deg -> out = (y, x) m; 1: in = (y, x) m -> out = (lat, lon) deg. */
int rdr_transform_tm(rdr_ctx* ctx, const double* params, int nparams, int direction, const double* in_a, const double* in_b, int64_t n,
                     double* out_a, double* out_b, int loc);
/* The same between EPSG:4326 and a CONIC model CRS (kind RDR_PROJ_LCC / RDR_PROJ_STERE, params as rdr_cube_set_projection): the
 * pyproj call of transformPoints(lats, lons, hgts, EPSG:4326, hrrr_proj) and back (test/test_delayFcns.py:67-84 round-trips it).
 * direction 0: in = (lat, lon) deg -> out = (y, x) m; 1: in = (y, x) m -> out = (lat, lon) deg. */
int rdr_transform_cone(rdr_ctx* ctx, int kind, const double* params, int nparams, int direction, const double* in_a, const double* in_b,
                       int64_t n, double* out_a, double* out_b, int loc);
/* Output grids in a PROJECTED CRS (out_proj = a UTM zone, an LCC or a polar-stereographic CRS; delay.py:207-209,259-263).
 * grid_kind RDR_GRID_TM: params as rdr_transform_tm; RDR_PROJ_LCC / RDR_PROJ_STERE: params as rdr_cube_set_projection.
 * rdr_grid_geodetic: lat[iy*nx+ix], lon[iy*nx+ix] (deg) of the node (ypts[iy], xpts[ix]) - `xx, yy = np.meshgrid(xpts, ypts)` then
 * transformPoints(yy, xx, ., grid CRS, EPSG:4326) (delay.py:261-263), bit for bit what rdr_transform_tm / rdr_transform_cone direction 1
 * return on the same nodes.  Axes and outputs at `loc`.  The origins of a ray-traced cube on such a grid (an LLH rdr_rays batch). */
#define RDR_GRID_TM 3
int rdr_grid_geodetic(rdr_ctx* ctx, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx, const double* ypts,
                      int64_t ny, double* lat, double* lon, int loc);
/* temporal blend, cli/raider.py:817-819: out = w1*a + w2*b (f32 cubes blend in f32, f64 in f64) */
int rdr_cube_blend(rdr_ctx* ctx, const rdr_cube* a, double w1, const rdr_cube* b, double w2, rdr_cube** out);
/* Azimuth-time-grid temporal interpolation.
 * rdr_inverse_time_weights = get_inverse_weights_for_dates (s1_azimuth_timing.py:326-399): az[n] = per-voxel acquisition
 * times and dates[nd] = model times, all in seconds on one epoch; weights[d*n + i] = normalised inverse-|dt| weight of
 * date d at voxel i, masked to |dt| <= window_s (window_s < 0: min_i |dates[i]-dates[0]|, the inferred model step).
 * RDR_ERR_INVALID: duplicate dates / no date ("No dates provided are within temporal window").
 * rdr_cube_blend_weighted = the combination of cli/raider.py:817-819 with those per-voxel weights: weights[d][nz*ny*nx]
 * in FILE order (z,y,x) (the shape of the reference's time grid), result a new f64 cube (a float64 weight array
 * promotes the f32 fields in the reference too). */
int rdr_inverse_time_weights(rdr_ctx* ctx, const double* az, int64_t n, const double* dates, int32_t nd, double window_s,
                             double regularizer, double* weights, int loc);
int rdr_cube_blend_weighted(rdr_ctx* ctx, const rdr_cube* const* cubes, int32_t nd, const double* weights, int loc, rdr_cube** out);
/* The whole 'azimuth_time_grid' branch of combine_weather_files (cli/raider.py:791-832, 891-916) in ONE pass, nothing in between
 * materialised: per voxel of the model grid lla2ecef of (lat2d, lon2d, z) -> zero-Doppler azimuth time + one-way range delay on the
 * orbit, truncated to milliseconds (get_azimuth_time_grid, s1_azimuth_timing.py:90-147; threshold 1e-7, <= 100 iterations) ->
 * the weights of rdr_inverse_time_weights -> the sums of rdr_cube_blend_weighted, bit for bit what those entries give on the same
 * time grid.  pointwise[nd] and / or total[nd] (either array may be NULL): the nd (1..8) model epochs, each array on one grid (shape,
 * dtype, bitwise-equal axes, projection; RDR_ERR_INVALID names the first epoch that differs) and both arrays on the same grid (their
 * dtypes may differ).  lat2d, lon2d: [ny*nx] degrees in the cubes' ascending axis order, at `loc`.  sv_t / sv_pos / sv_vel: the state
 * vectors as rdr_orbit_look_vectors takes them (HOST; strictly increasing; 4 <= nsv <= 320, the table the kernel keeps in LDS).
 * dates_s[nd]: model times in seconds relative to dates[0]; window_s / reg as rdr_inverse_time_weights; offset_us = (the epoch sv_t
 * counts from, truncated to milliseconds) - dates[0], in microseconds.  *out_pointwise / *out_total: new f64 cubes with epoch 0's
 * axes and projection (NULL where the source array is NULL).  time_grid (may be NULL): [nz][ny][nx] acquisition times in seconds
 * relative to dates[0], at `loc`.  *flags (HOST; the call synchronises): bit 0 = a voxel's solve failed or left the orbit span (its
 * outputs are NaN: "The Time Grid return nans", cli/raider.py:913-914), bit 1 = no date lay inside the window anywhere ("No dates
 * provided are within temporal window"). */
int rdr_cube_blend_azimuth_time(rdr_ctx* ctx, const rdr_cube* const* pointwise, const rdr_cube* const* total, int32_t nd, const double* lat2d,
                                const double* lon2d, int loc, const double* sv_t, const double* sv_pos, const double* sv_vel, int64_t nsv,
                                const double* dates_s, double window_s, double reg, int64_t offset_us, rdr_cube** out_pointwise,
                                rdr_cube** out_total, double* time_grid, int32_t* flags);

/* GUNW radian conversion (aria/calcGUNW.py:54-59): out = delay * (-4 pi / wavelength) for both fields;
 * dtype RDR_F32 multiplies in f32 by the f32-rounded factor (NumPy weak-scalar rule), RDR_F64 in f64.  In place allowed. */
int rdr_delays_to_phase(rdr_ctx* ctx, const void* wet, const void* hydro, int64_t n, int dtype, double wavelength,
                        void* wet_out, void* hydro_out, int loc);

/* copy the (blended) fields back, (y,x,z) C-order, dtype of the cube */
int rdr_cube_read(rdr_ctx* ctx, const rdr_cube* cube, void* wet, void* hydro);

/* ---- zenith / projected path -----------------------------------------------------------------
 * scipy RegularGridInterpolator.__call__ on both fields (delay.py:214,120-121): pts[n,3] = (y,x,z). */
/* Either of wet / hydro may be NULL: that field is then neither stored nor downloaded (a caller that evaluates the two interpolators one
 * after the other - `for intp in interpolators: intp(pts)`, delay.py:213-214 - moves 8 B per point and call instead of 16). */
int rdr_interp3(rdr_ctx* ctx, const rdr_cube* cube, const double* pts, int64_t n, double* wet,
                double* hydro, int loc);
/* The second stage of tropo_delay's point branch (delay.py:110-128) in one call: the gather of rdr_interp3 on the intermediate delay
 * cube and, for a projected line of sight, the division of Conventional.__call__ (losreader.py:130-133) before the values leave the
 * device - 24-32 B per point up, 16 B down, nothing in between.
 * Points: three arrays y[n], x[n], z[n] (what aoi.readLL() / readZ() hand out: no packed copy on the host), or y = packed pts[n,3]
 * with x = z = NULL.  proj_mode 0: no projection; 1: proj[n] = incidence angles (deg), delay / cosd(inc) (inc_hd_to_enu(...)[..., -1],
 * losreader.py:374-396); 2: one incidence inc0 for every point (proj unused); 3: proj[n] = the divisor itself (the cosine of the look
 * angle state_to_los returns for an orbit file, losreader.py:122-128).  Either output may be NULL. */
int rdr_interp3_project(rdr_ctx* ctx, const rdr_cube* cube, const double* y, const double* x, const double* z, int64_t n, int proj_mode,
                        const double* proj, double inc0, double* wet, double* hydro, int loc);
/* Large random point sets on a cube beyond the caches (BASELINE configs[4]: 5 M stations on a 1000 x 1000 x 50 cube): rdr_interp3
 * then reads four 128 B lines per point for 16 B each.  The cube can carry a second, cell-column-major copy ("corner quads",
 * 5.3 x its bytes for f32, 8 x for f64) from which a point's eight corners are ONE line - same values, same arithmetic, 3.3 x less
 * HBM traffic.  mode 1: build it now; mode 0: free it.  Without this call rdr_interp3 builds it by itself from the second call with
 * >= 262144 points on a cube beyond 192 MB (the Infinity Cache holds smaller ones) - or at the first, when the point set is large enough that the build pays for itself within
 * that call (n x 175 B > the copy's bytes, from the measured rates) - if it fits a quarter of the free memory (env
 * RAIDER_HIP_POINT_INDEX=0 never, =1 at the first such call, =2 second call only).  rdr_cube_point_index_bytes: bytes the copy holds now (0: none). */
int rdr_cube_point_index(rdr_ctx* ctx, rdr_cube* cube, int mode);
int64_t rdr_cube_point_index_bytes(const rdr_cube* cube);
/* _build_cube (delay.py:196-216) for model_crs == pts_crs: out[(iz*ny+iy)*nx+ix] = f(ypts[iy],xpts[ix],zpts[iz]) */
int rdr_build_cube(rdr_ctx* ctx, const rdr_cube* cube, const double* xpts, int64_t nx, const double* ypts,
                   int64_t ny, const double* zpts, int64_t nz, double* wet, double* hydro, int loc);
/* rdr_build_cube on an output grid in a projected CRS (grid_kind / params as rdr_grid_geodetic): replaces the per-height loop of
 * delay.py:205-215 (transformPoints(yy, xx, ht, pts_crs, model_crs) + the interpolator calls).  The nodes are transformed once - the
 * projection is 2-D - by the transform kernels, to lon/lat or, for a cube that carries a projection (rdr_cube_set_projection /
 * rdr_cube_view: the model CRS), on to the model's cone; the gather is rdr_build_cube's.  Same bits as that loop. */
int rdr_build_cube_grid(rdr_ctx* ctx, const rdr_cube* cube, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx,
                        const double* ypts, int64_t ny, const double* zpts, int64_t nz, double* wet, double* hydro, int loc);
/* 1 / 0: the result of the last rdr_build_cube call with HOST arrays on this ctx holds / does not hold a NaN - the scan the caller
 * runs over the result (delay.py:187) done on the device before the download; -1: unknown (no such call yet, or device arrays). */
int rdr_last_nan_output(rdr_ctx* ctx);
/* _build_cube whose result STAYS on the device as a new float64 cube with axes (ypts, xpts, zpts) - the intermediate delay cube of
 * tropo_delay's point branch (delay.py:96-121: _get_delays_on_cube -> writeResultsToXarray -> getInterpolators(ds, 'ztd')), ready
 * for rdr_interp3_project.  Nothing crosses PCIe but the three axes.  rdr_cube_has_nan(*out) answers the scan of delay.py:187
 * ("There are missing delay values").  Needs two nodes per axis (scipy's grid rule), nz <= 512. */
int rdr_build_cube_to_cube(rdr_ctx* ctx, const rdr_cube* cube, const double* xpts, int64_t nx, const double* ypts, int64_t ny,
                           const double* zpts, int64_t nz, int loc, rdr_cube** out);
/* rdr_build_cube_to_cube on an output grid in a projected CRS (as rdr_build_cube_grid); the new cube's axes are (ypts, xpts, zpts) in
 * that CRS. */
int rdr_build_cube_grid_to_cube(rdr_ctx* ctx, const rdr_cube* cube, int grid_kind, const double* params, int nparams, const double* xpts,
                                int64_t nx, const double* ypts, int64_t ny, const double* zpts, int64_t nz, int loc, rdr_cube** out);
/* rdr_interp3 on the two-epoch temporal blend w1 * a + w2 * b (cli/raider.py:817-819) WITHOUT making the blended cube: the blend is
 * applied at the eight corners of every point, in the cubes' own dtype with blend_kernel's arithmetic - the same bits as rdr_cube_blend
 * followed by rdr_interp3.  It reads eight lines per point instead of four and none of the blend's 24 B per cell: the better deal for a
 * point set below ~5 % of the cube's cells - the station block of one rank of a multi-GPU job (BASELINE configs[4]), where a replicated
 * blend is what stops the job from scaling.  Points as rdr_interp3_project (three arrays, or y = packed pts[n,3] with x = z = NULL). */
int rdr_interp3_blend(rdr_ctx* ctx, const rdr_cube* a, double w1, const rdr_cube* b, double w2, const double* y, const double* x, const double* z,
                      int64_t n, double* wet, double* hydro, int loc);
/* The same query when the point set is LARGE against the cube (one GPU holding all 5 M stations of BASELINE configs[4]): the blend is made
 * as a cube after all - 24 B per cell, as rdr_cube_blend - but into the context's scratch and in the layout the gather reads best
 * (neighbouring x columns paired: 3 cache lines per random point on average instead of 4), then gathered in the same call.  The paired
 * cube never becomes an rdr_cube, so nothing else can be handed that layout.  Same arithmetic as rdr_cube_blend + rdr_interp3
 * (cli/raider.py:817-819, delay.py:116-121): the same bits.  Points / outputs as rdr_interp3_blend. */
int rdr_interp3_blend_cube(rdr_ctx* ctx, const rdr_cube* a, double w1, const rdr_cube* b, double w2, const double* y, const double* x, const double* z,
                           int64_t n, double* wet, double* hydro, int loc);
/* tropo_delay's point branch for a zenith / projected line of sight (delay.py:96-128) in ONE call, host arrays in, host arrays out:
 * rdr_build_cube_to_cube on the output grid (xpts[nx], ypts[ny], zpts[nz]) + rdr_interp3_project at the query points, with the
 * intermediate cube in the context's scratch (no allocation per call) and the upload of the points running under its build.  Same
 * kernels and arithmetic as the two separate entries: the same bits.  Points / projection / outputs as rdr_interp3_project;
 * *cube_has_nan (may be NULL): the intermediate cube holds a NaN - the scan of delay.py:187 ("There are missing delay values"). */
int rdr_point_delays(rdr_ctx* ctx, const rdr_cube* cube, const double* xpts, int64_t nx, const double* ypts, int64_t ny, const double* zpts,
                     int64_t nz, const double* y, const double* x, const double* z, int64_t n, int proj_mode, const double* proj, double inc0,
                     double* wet, double* hydro, int32_t* cube_has_nan);
/* rdr_point_delays with the intermediate grid in a projected CRS (grid_kind / params as rdr_grid_geodetic; the query points y, x, z
 * in that CRS): the point branch of delay.py:96-128 for out_proj = UTM / LCC / polar stereographic in one call (the reference's
 * per-height loop delay.py:205-215 for the cube, then the gather). */
int rdr_point_delays_grid(rdr_ctx* ctx, const rdr_cube* cube, int grid_kind, const double* params, int nparams, const double* xpts, int64_t nx,
                          const double* ypts, int64_t ny, const double* zpts, int64_t nz, const double* y, const double* x, const double* z, int64_t n,
                          int proj_mode, const double* proj, double inc0, double* wet, double* hydro, int32_t* cube_has_nan);
/* A DATE SERIES at query points: rdr_interp3_project on `ncubes` cubes of one grid (same shape, dtype, bitwise-equal axes and
 * projection, as rdr_raytrace_slices_epochs: RDR_ERR_INVALID names the first epoch that differs) in one pass - the second stage of
 * the point branch (delay.py:110-128) for every date of the loop of cli/raider.py:159-400.  The points - and a shared proj - go up
 * once; per point the cell search, the weights and the address are made once, then eight corner loads and scipy's sum
 * (_rgi.py:490-498) per epoch, up to four epochs per launch: epoch e's values are bit for bit rdr_interp3_project's on cubes[e].
 * wet / hydro: [ncubes][n].  proj_stride 0: one proj[n] for every epoch; n: proj[ncubes][n] (Conventional with an orbit file calls
 * setTime per date, losreader.py:122-128: its divisor may differ by date).  Host arrays of >= 2^18 points are chunked through the
 * three-stream pipeline of rdr_interp3_project.  ncubes == 1 is rdr_interp3_project itself.  loc == RDR_DEVICE: nothing is uploaded,
 * and the one-cube gather per date measured faster than the stacked one (profiles/r13_point_series_before_routing.json), so the entry
 * runs rdr_interp3_project's kernels date by date. */
int rdr_interp3_project_epochs(rdr_ctx* ctx, const rdr_cube* const* cubes, int32_t ncubes, const double* y, const double* x, const double* z,
                               int64_t n, int proj_mode, const double* proj, int64_t proj_stride, double inc0, double* wet, double* hydro, int loc);
/* rdr_point_delays / rdr_point_delays_grid for a date series (delay.py:96-128 per date): the ncubes intermediate cubes are built one
 * after the other into one scratch allocation (RDR_ERR_OOM when it does not fit: go date by date), the points travel up once under the
 * first build, one gather pass serves every date.  nparams 0: the output grid is in lon/lat or the model CRS (rdr_point_delays:
 * grid_kind / params unused); else grid_kind / params as rdr_point_delays_grid.  wet / hydro: [ncubes][n]; proj / proj_stride as
 * rdr_interp3_project_epochs; cube_has_nan[ncubes] (may be NULL): the scan of delay.py:187 per date.  Host arrays in, host arrays out. */
int rdr_point_delays_epochs(rdr_ctx* ctx, const rdr_cube* const* cubes, int32_t ncubes, int grid_kind, const double* params, int nparams,
                            const double* xpts, int64_t nx, const double* ypts, int64_t ny, const double* zpts, int64_t nz, const double* y,
                            const double* x, const double* z, int64_t n, int proj_mode, const double* proj, int64_t proj_stride, double inc0,
                            double* wet, double* hydro, int32_t* cube_has_nan);
/* Host bytes of query points and divisors copied to the device since the last of the two calls above began, counted where the copies
 * are issued (diagnostics: a series uploads its points once, not once per date); -1: NULL context. */
int64_t rdr_point_upload_bytes(const rdr_ctx* ctx);
/* Conventional.__call__ tail (losreader.py:130-133): delay / cosd(inc) in place, inc[n] in degrees (what inc_hd_to_enu(...)[..., -1]
 * holds for an incidence raster).  The reference projects wet and hydro in two calls: either pointer may be NULL. */
int rdr_project_cosinc(rdr_ctx* ctx, double* wet, double* hydro, const double* inc, int64_t n, int loc);
/* The same with the divisor given (losreader.py:130-131: LOS_enu from an orbit file is cos(look angle), same shape as the delays). */
int rdr_project_divide(rdr_ctx* ctx, double* wet, double* hydro, const double* divisor, int64_t n, int loc);

/* ---- ray-traced path --------------------------------------------------------------------------
 * rdr_ray_levels: the slice-uniform part of build_ray (losreader.py:785-808).  lo/hi/kz need room for
 * nz-1 entries; kz[k] = index of the model interval. Returns RDR_ERR_NO_LEVELS when K==0. */
int rdr_ray_levels(const rdr_cube* cube, double ht, double zref, int32_t* K, double* lo, double* hi, int32_t* kz);
/* Pass 1 (build_ray, losreader.py:772-835, fused - nothing materialised): per-level max ray length over
 * the batch (what delay.py:283 reduces) and the RDR_FLAG_* bits.  maxlen (K doubles) and flags are HOST
 * outputs (this call synchronises).  Multi-GPU callers all-reduce MAX(maxlen) / OR(flags) across ranks. */
int rdr_ray_prepass(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, double ht, double zref,
                    double* maxlen, int32_t* flags);
/* nParts = ceil(maxlen/max_seg)+1 (delay.py:283) */
int rdr_nparts(const double* maxlen, int32_t K, double max_seg, int32_t* nparts);
/* Device-resident variant of the prepass / march pair for multi-GPU slabs: `partition` is a DEVICE buffer of
 * K+4 doubles - the per-level maxima of the ray length followed by the four RDR_FLAG_* bits as 0.0 / 1.0 - so that the
 * caller can run ONE element-wise MAX all-reduce (RCCL) on it between the two calls and no host round trip happens at all.
 * Rays, outputs and the partition must live on the device; both calls are asynchronous on the ctx stream.  The march
 * derives nParts = ceil(max/max_seg)+1 (delay.py:283) on the device; error conditions (all-NaN, diverged) are not
 * reported here (the outputs are NaN) - use rdr_ray_prepass when they must be. */
int rdr_ray_prepass_device(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, double ht, double zref, double* partition);
int rdr_ray_march_device(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, double ht, double zref, double max_seg,
                         const double* partition, double* wet, double* hydro);

/* The level table pass 2 reads (tests, diagnostics): per slice hts[s] nz+1 records of 80 bytes - the slice's K levels, a weight-0
 * sentinel behind the last one, zeros after it - written by the kernel that writes it before every pass 2.  A record is, in order,
 * the doubles xv, hs, step, zmid, r0, r1, gk, rk (abscissa of the level's top in the crossing polynomial; 0.5e-6/(nParts-1);
 * 1/(nParts-1); node g[zb+1] under the level's top and 1/(g[zb+1]-g[zb]), 1/(g[zb+2]-g[zb+1]), zb = clamp(kz, 0, nz-3); g[kz] and
 * 1/(g[kz+1]-g[kz])), then int32 npkz = nParts | kz << 17 and three zero int32.  The partition is given as rdr_ray_march takes it,
 * nparts[nslices][ld] (maxlen NULL), or as pass 1 leaves it, length maxima maxlen[nslices][ld] with max_seg (nparts NULL);
 * nz-1 <= ld <= 512.  records: HOST buffer of nslices * (nz+1) * 80 bytes.  Synchronises. */
int rdr_level_table(rdr_ctx* ctx, const rdr_cube* cube, const double* hts, int32_t nslices, double zref, const int32_t* nparts,
                    const double* maxlen, int32_t ld, double max_seg, void* records);

/* Pass 2 (delay.py:285-323 + build_ray recomputed in registers): trapezoid integral of both fields along
 * each ray with the GIVEN partition nparts[K] (host array) and clamp decision `flags`.
 * wet/hydro: [n] outputs (overwritten, not accumulated), location = rays->loc. */
int rdr_ray_march(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, double ht, double zref,
                  const int32_t* nparts, int32_t flags, double* wet, double* hydro);
/* One slice of _build_cube_ray (delay.py:256-323): prepass -> nParts on device -> march, no host
 * round trip.  nparts_out (host, K entries, may be NULL) and flags_out (may be NULL) are filled after
 * the launch (this forces a synchronisation; pass NULL for a fully asynchronous call with RDR_DEVICE).
 * Returns RDR_ERR_ALL_NAN / RDR_ERR_NAN_LENGTH only when it synchronised. */
int rdr_raytrace(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, double ht, double zref,
                 double max_seg, double* wet, double* hydro, int32_t* nparts_out, int32_t* flags_out);

/* The height loop of _build_cube_ray (delay.py:256-323) in one call: `nslices` slices at heights hts[] (host array) of the SAME
 * origins - GRID or LLH - each integrated exactly as rdr_raytrace would (its own level table, per-level slice maxima, nParts and
 * z-clamp decision), but in one pass-1 / pass-2 launch pair, so that production-sized jobs (20 heights x 1e4-1e5 rays,
 * aria/prepFromGUNW.py:173,180) fill the GPU.  los_per_slice != 0: rays->los / inc / hd hold nslices consecutive blocks of
 * rays->n entries (look vectors that depend on the target height, losreader.py:219-255); 0: one block serves every slice.
 * wet / hydro: [nslices][n].  Host outputs, filled after a synchronisation when given: K_out[nslices] contributing model
 * intervals per slice (0: build_ray -> None, the slice's delays are 0), nparts_out[nslices][ld] (ld >= nz-1),
 * flags_out[nslices] RDR_FLAG_* bits - the caller raises what delay.py:276-283 raises, slice by slice. */
int rdr_raytrace_slices(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, const double* hts, int32_t nslices,
                        int32_t los_per_slice, double zref, double max_seg, double* wet, double* hydro, int32_t* K_out,
                        int32_t* nparts_out, int32_t ld, int32_t* flags_out);

/* rdr_raytrace_slices whose delays STAY on the device as a new float64 cube with axes (rays->ypts, rays->xpts, hts): the intermediate
 * cube of tropo_delay's point branch for a ray-traced line of sight (delay.py:96-121).  GRID batches, or LLH batches of a projected
 * output grid (origins from rdr_grid_geodetic) that carry the grid's axes in xpts[nx] / ypts[ny] with n == nx * ny; >= 2 nodes per
 * axis, strictly monotonic hts; the partition outputs are as for rdr_raytrace_slices. */
int rdr_raytrace_slices_to_cube(rdr_ctx* ctx, const rdr_cube* cube, const rdr_rays* rays, const double* hts, int32_t nslices,
                                int32_t los_per_slice, double zref, double max_seg, int32_t* K_out, int32_t* nparts_out, int32_t ld,
                                int32_t* flags_out, rdr_cube** out);

/* A time series (cli/raider.py:159-400 loops calcDelays over dates with one AOI and one LOS): rdr_raytrace_slices of the SAME ray
 * batch through ncubes weather epochs cubes[0..ncubes-1] in one call.  Pass 1 - the ray polynomials, level crossings and the slice
 * partition - runs once per chunk whatever ncubes is; pass 2 marches up to four epochs together (one cell search and address per
 * sample, one corner gather per epoch).  Epoch e's delays are bit for bit those of rdr_raytrace_slices on cubes[e].
 * The cubes must share shape, dtype, bitwise-equal axes and the projection (else RDR_ERR_INVALID naming the first epoch that
 * differs); rays with per-ray heights (rays->hts) are refused (rdr_raytrace_epochs takes them).  wet / hydro: [ncubes][nslices][n].  K_out[nslices] and
 * nparts_out[nslices][ld] are shared by every epoch (the partition depends on geometry and levels only); flags_out[ncubes][nslices]:
 * the partition bits are equal across epochs, RDR_FLAG_NAN_OUTPUT is the epoch's own.  ncubes == 1 is rdr_raytrace_slices. */
int rdr_raytrace_slices_epochs(rdr_ctx* ctx, const rdr_cube* const* cubes, int32_t ncubes, const rdr_rays* rays, const double* hts,
                               int32_t nslices, int32_t los_per_slice, double zref, double max_seg, double* wet, double* hydro,
                               int32_t* K_out, int32_t* nparts_out, int32_t ld, int32_t* flags_out);

/* rdr_raytrace_slices_epochs whose delays stay on the device: out[ncubes] new float64 cubes with axes (rays->ypts, rays->xpts, hts),
 * as rdr_raytrace_slices_to_cube makes one - the intermediate cubes of a series of station queries.  The batches rdr_raytrace_slices_to_cube
 * takes. */
int rdr_raytrace_slices_epochs_to_cubes(rdr_ctx* ctx, const rdr_cube* const* cubes, int32_t ncubes, const rdr_rays* rays,
                                        const double* hts, int32_t nslices, int32_t los_per_slice, double zref, double max_seg,
                                        int32_t* K_out, int32_t* nparts_out, int32_t ld, int32_t* flags_out, rdr_cube** out);

/* A time series on ONE ray batch with ONE height per ray: rdr_raytrace of the same batch through ncubes weather epochs - a SAR scene
 * on a DEM (rays->hts, `ht` <= min(hts) as for rdr_raytrace) traced for every acquisition date, or a plain batch at height `ht`.
 * GRID, LLH and XYZ origins, every LOS mode.  Pass 1 - ray polynomials, level crossings, the per-level maxima, every ray's first
 * level - runs once (per chunk when the ray records exceed the workspace limit); pass 2 marches up to four epochs together: per
 * sample one set of polynomial evaluations, one cell search and one element offset, then one corner gather per epoch.  Epoch e's
 * delays are bit for bit those of rdr_raytrace on cubes[e].  The cubes must share shape, dtype, bitwise-equal axes and the
 * projection (else RDR_ERR_INVALID naming the first epoch that differs).  wet / hydro: [ncubes][n], epoch-major.  nparts_out[K] and
 * *flags_out (either may be NULL; a device batch then stays asynchronous) belong to pass 1 and are shared by every epoch, as
 * rdr_raytrace returns them; statuses are rdr_raytrace's.  ncubes == 1 is rdr_raytrace; only then is a large host batch uploaded
 * through the pipelined path. */
int rdr_raytrace_epochs(rdr_ctx* ctx, const rdr_cube* const* cubes, int32_t ncubes, const rdr_rays* rays, double ht, double zref,
                        double max_seg, double* wet, double* hydro, int32_t* nparts_out, int32_t* flags_out);

/* Materialising variants for API parity on small inputs:
 * getTopOfAtmosphere (losreader.py:706-733): factor==NULL -> 10 iterations with factor 1, else 3 */
int rdr_top_of_atmosphere(rdr_ctx* ctx, const double* xyz, const double* los, int64_t n, double toaheight,
                          const double* factor, double* pos, int loc);
/* build_ray (losreader.py:772-835): ray_lengths[K,n], low[K,n,3], high[K,n,3] */
int rdr_build_ray(rdr_ctx* ctx, const double* model_zs, int64_t nz, double ht, const double* xyz,
                  const double* los, int64_t n, double zref, int32_t* K, double* lengths, double* low,
                  double* high, int loc);

/* ---- geodesy helpers (pyproj call sites utilFcns.py:77-88; LOS helpers losreader.py:302-316,374-396) */
int rdr_lla2ecef(rdr_ctx* ctx, const double* lat, const double* lon, const double* h, int64_t n, double* xyz, int loc);
int rdr_ecef2lla(rdr_ctx* ctx, const double* xyz, int64_t n, double* lon, double* lat, double* h, int loc);
/* look vectors for a ray batch (any los_mode) -> los[n,3] */
int rdr_look_vectors(rdr_ctx* ctx, const rdr_rays* rays, double ht, double* los);

/* Front end of the cube producer for ECMWF hybrid model levels (ERA-5, HRES): utilFcns.calcgeoh (:781-859) +
 * utilFcns.geo_to_ht (:378-410) + the re-ordering of models/ecmwf.py:92-110.  z_surf (surface geopotential) and lnsp: [ny*nx] f32;
 * t, q: [nlev, ny, nx] f32 with level 1 = model top (file order); lats[ny] f32; a, b: [nlev+1] hybrid coefficients (host).
 * p_out, zs_out: [ny, nx, nlev] f64, BOTTOM level first - the layout rdr_cubes_from_model_levels takes.  Arithmetic is float64
 * on the float32 inputs: the reference's float32 evaluation of these formulas is ill-conditioned (heights off by up to 2.4 m,
 * platform dependent in the last bit of logf); DESIGN.md 6.5. */
int rdr_ecmwf_model_levels(rdr_ctx* ctx, const float* z_surf, const float* lnsp, const float* t, const float* q, const float* lats,
                           const double* a, const double* b, int32_t nlev, int64_t ny, int64_t nx, double R_d,
                           double* p_out, double* zs_out, int loc);

/* Front end of the cube producer for states on pressure levels, or on levels that carry their own height field: ERA-5 / HRES
 * pressure-level files (models/ecmwf.py:252-303), and the same steps where other providers take them (geopotential height with 2-D
 * latitudes on a projected grid; geometric heights with a 3-D pressure field).  Inputs in FILE layout [nlev, ny, nx], x contiguous,
 * all f64: height with height_kind 0 = geopotential m2 s-2, divided by g0 (ecmwf.py:284), 1 = geopotential height m - both then
 * through WeatherModel._get_heights (weatherModel.py:326-330) = utilFcns.geo_to_ht (:378-410) - 2 = geometric height m, moved only;
 * p: p_ndim 1 = the level list [nlev] in Pa, broadcast (ecmwf.py:292), 3 = a field; t; hum (q or rh, moved only); lats: lat_ndim
 * 1 = [ny], 2 = [ny, nx], in the file's row / column order.  top_first: level 0 of the file is the top (else the surface);
 * rows_descending / cols_descending: latitudes / longitudes run downwards in the file (ecmwf.py:264-275).
 * zs_out, p_out, t_out, hum_out: [ny, nx, nlev] f64, levels surface -> top, rows and columns ascending (ecmwf.py:295-303) - the
 * layout rdr_cubes_from_model_levels takes.  Inputs live at `loc`, outputs at `out_loc` (host in -> device out feeds the producer
 * without a round trip). */
int rdr_pressure_level_state(rdr_ctx* ctx, const double* height, int height_kind, const double* p, int p_ndim, const double* t,
                             const double* hum, const double* lats, int lat_ndim, int64_t nlev, int64_t ny, int64_t nx,
                             int top_first, int rows_descending, int cols_descending, double* zs_out, double* p_out,
                             double* t_out, double* hum_out, int loc, int out_loc);

/* Cube producer (models/weatherModel.py:235-262: _find_e -> _uniform_in_z -> _checkForNans -> wet/hydro refractivity ->
 * _adjust_grid -> _getZTD): model-level columns zs3/p/t/hum [ny, nx, nlev] (heights ascending along the last axis,
 * humidity_type 0 = specific humidity q, 1 = relative humidity %) are resampled to the uniform levels new_z[nz] and
 * turned into the two device cubes the delay kernels read, without a NetCDF round trip:
 *   *pointwise = (wet, hydro) refractivity, f32;   *total = (wet_total, hydro_total) zenith delays, f64.
 * When zmin < new_z[0] an extra bottom level at zmin is added (the reference's padLower).  t_out/p_out/e_out (f32,
 * [ny, nx, nz_out], all three or none) return the resampled state for parity checks.  k1,k2,k3: models/ecmwf.py:26-28. */
int rdr_cubes_from_model_levels(rdr_ctx* ctx, const double* ys, int64_t ny, const double* xs, int64_t nx, const double* zs3,
                                const double* p, const double* t, const double* hum, int humidity_type, int64_t nlev,
                                const double* new_z, int64_t nz, double k1, double k2, double k3, double zmin, int loc,
                                rdr_cube** pointwise, rdr_cube** total, float* t_out, float* p_out, float* e_out);

/* Look vectors from orbit state vectors: replaces the per-pixel isce3 geo2rdr + Orbit.interpolate loop of
 * Raytracing.getLookVectors (losreader.py:219-255; zero-Doppler, threshold 1e-7, maxiter 30 at the call site).
 * sv_t[nsv] seconds (strictly increasing, HOST), sv_pos/sv_vel [nsv,3] ECEF (HOST); xyz[n,3] targets, los[n,3] unit
 * vectors target->sensor (NaN where the solve fails or leaves the orbit span); aztime / srange optional [n].
 * isce3 itself is not available to this build: parity with it is UNPINNED (the algorithm is restated from its
 * published description). */
int rdr_orbit_look_vectors(rdr_ctx* ctx, const double* sv_t, const double* sv_pos, const double* sv_vel, int64_t nsv,
                           const double* xyz, int64_t n, double threshold, int maxiter, double* los, double* aztime,
                           double* srange, int loc);

/* ---- the reference's two native extensions ----------------------------------------------------
 * RAiDER.interpolate.interpolate (tools/bindings/interpolate/src/module.cpp:26-294, interpolate.cpp):
 * N-D linear interpolation (ndim <= 8 on device), C-order values, interp_points[n,ndim].
 * has_fill: queries with upper-bound index outside [1, N-1] (incl. ON the last node) get fill_value;
 * else indices are clamped (linear extrapolation).  interpolate.h:23-74 */
int rdr_interp_nd(rdr_ctx* ctx, int32_t ndim, const double* const* axes, const int64_t* axis_len,
                  const double* values, const double* interp_points, int64_t n, int has_fill,
                  double fill_value, double* out, int loc);
/* RAiDER.interpolate.interpolate_along_axis (module.cpp:296-493, interpolate.cpp:260-332) on arrays made
 * contiguous with the axis LAST: points/values [ncol, m], interp_points/out [ncol, mq]. */
int rdr_interp_along_axis(rdr_ctx* ctx, const double* points, const double* values, int64_t ncol, int64_t m,
                          const double* interp_points, int64_t mq, int has_fill, double fill_value,
                          double* out, int loc);
/* RAiDER.makePoints.makePoints{0,1,2,3}D (tools/bindings/utils/makePoints.pyx:15-148):
 * out[r,3,npts] = sp[r,c] + (k*step)*slv[r,c]; npts = rdr_make_points_count(max_len, step) */
int64_t rdr_make_points_count(double max_len, double step);
int rdr_make_points(rdr_ctx* ctx, double max_len, const double* sp, const double* slv, int64_t nrays,
                    double step, double* out, int loc);

/* ---- georeferenced rasters: AOI bounds and DEM heights (llreader.py, interpolator.py:133-184) -----------------------------------
 * rdr_raster_sample = interpolateDEM / interpolate_elevation: a north-up raster[height][width] of dtype RDR_I16 / RDR_F32 / RDR_F64
 * with GDAL geotransform gt6 (HOST; gt6[2] == gt6[4] == 0, gt6[1] and gt6[5] non-zero of either sign) sampled at (x[i], y[i]) in the
 * raster's CRS.  method 0 = nearest: the pixel whose cell holds the point, col = floor((x - gt0) / gt1), row = floor((y - gt3) / gt5)
 * in f64 - rasterio.transform.rowcol's default (interpolator.py:173); NaN where row / col fall outside or a coordinate is NaN.
 * method 1 = bilinear on pixel-centre coordinates (da_dem.interp(y=, x=), interpolator.py:149) with scipy's cell rule and sum
 * order; NaN outside the hull of the centres, the last centre inside; needs two pixels per axis.  has_nodata: a raster value equal
 * to `nodata` counts as NaN (the reference passes no-data values through: has_nodata = 0).  raster, x, y and out live at `loc`.
 * RDR_ERR_INVALID: NULL, height / width / n <= 0, an unknown dtype / method / loc, a rotated or degenerate geotransform. */
int rdr_raster_sample(rdr_ctx* ctx, const void* raster, int dtype, int64_t height, int64_t width, const double* gt6, const double* x,
                      const double* y, int64_t n, int method, int has_nodata, double nodata, double* out, int loc);
/* The statistics bounds_from_latlon_rasters takes from rio_stats (llreader.py:397-420, utilFcns.py:213-241) for one raster or two of
 * equal length (b may be NULL) in one pass: out6 = {min a, max a, valid a, min b, max b, valid b}, valid = elements that are neither
 * NaN nor (has_nodata) equal to `nodata`, as a double; min / max are NaN where valid is 0 (and for a NULL b).  Minima and maxima are
 * exact and no floating-point atomics are used: the same bytes on every run.  a, b and out6 live at `loc`. */
int rdr_raster_bounds(rdr_ctx* ctx, const void* a, const void* b, int dtype, int64_t n, int has_nodata, double nodata, double* out6, int loc);

/* ---- GeoTIFF segments (raider_amd/tifflite.py): tiles and strips decoded and put together on the device ---------------------------
 * rdr_tiff_lzw_decode: `nseg` independent TIFF-flavoured LZW streams (MSB-first codes of 9 - 12 bits, Clear = 256, EOI = 257,
 * libtiff's early change of the code width) out of one byte buffer `src` of `src_bytes`: stream i is src[seg_offset[i] ..
 * + seg_bytes[i]) and is written to out + i * out_stride, at most seg_out_bytes[i] <= out_stride bytes of it; bytes of a slot the
 * stream does not reach keep their value.  status[i]: 0 = the stream ended with EOI, or ended exactly as its slot was full;
 * 1 = the input ended before EOI with the slot not full, or the stream holds more than the slot takes; 2 = a code beyond the
 * table.  A bad stream sets its status and stops; nothing is read outside its segment or written outside its slot.  src, out and
 * status live at `loc`; the three int64 tables are HOST arrays.  One wave per segment, the string table in LDS; strings are
 * expanded from the table and the output is never read back.  RDR_ERR_INVALID: NULL, sizes <= 0, a segment outside src, a slot
 * beyond out_stride, out_stride >= 2 GiB. */
int rdr_tiff_lzw_decode(rdr_ctx* ctx, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                        const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int loc);
/* rdr_tiff_assemble: decoded segments (segment k at segs + k * seg_stride, seg_stride a multiple of 8; file order: left to right, top
 * to bottom, plane after plane for planar = 2) -> the raster out[height][width] of band `band` (0-based), or out[bands][height][width]
 * for band = -1, in native byte order.  Segments are tile_h x tile_w pixels (strips: tile_w = width, tile_h = RowsPerStrip, the
 * last strip may be short); padding right of `width` and below `height` is clipped.  swap != 0: samples are byte-swapped first;
 * predictor 2: each segment row is then summed along x per band, modulo 2^(8 * sample_bytes) (NumPy's cumsum in the unsigned type).
 * sample_bytes 1 / 2 / 4 / 8: samples travel as bits, so every TIFF sample type of that size is served.  No predictor, no swap and
 * one strip (per plane) covering the raster is a plain copy.  segs and out live at `loc`. */
int rdr_tiff_assemble(rdr_ctx* ctx, const void* segs, int64_t seg_stride, int64_t height, int64_t width, int64_t tile_h, int64_t tile_w,
                      int predictor, int swap, int sample_bytes, int planar, int bands, int band, void* out, int loc);
/* rdr_tiff_predict: what rdr_tiff_assemble's predictor 2 undoes - out[y][x] = in[y][x] - in[y][x-1] along every row of `width` samples,
 * modulo 2^(8 * sample_bytes); the first sample of a row is kept.  in and out are different buffers at `loc`. */
int rdr_tiff_predict(rdr_ctx* ctx, const void* in, int sample_bytes, int64_t height, int64_t width, void* out, int loc);

/* ---- zlib streams written on the device (raider_amd/deflate.py; csrc/deflate_kernels.h) --------------------------------------------
 * rdr_deflate_bound(n): the largest stream rdr_deflate_encode makes of n bytes: n + 5 * ceil(n / 32768) + 6 <= n + n / 2048 + 32.
 * rdr_deflate_encode: `nseg` independent byte ranges src[seg_offset[i] .. + seg_bytes[i]) (any byte offset) -> one complete zlib
 * stream each (RFC 1950 / 1951: 78 01, deflate blocks, the big-endian Adler-32 of the range), packed back to back into `out` in
 * segment order; out_offset[i] = where stream i starts, out_offset[nseg] = the total (HOST array of nseg + 1).  The call
 * synchronises.  Every 32 KiB sub-block of a range is encoded by one wave, independently of all others (no match reaches across a
 * sub-block start), as one fixed-Huffman block closed by an empty stored block, or as a stored block when that is not smaller;
 * dynamic Huffman tables are not written.  The same input gives the same bytes on every run.  src and out live at `loc`, the
 * tables are HOST arrays.  RDR_ERR_INVALID (and nothing written): NULL, a segment outside src, seg_bytes[i] <= 0, out_capacity
 * below the sum of rdr_deflate_bound(seg_bytes[i]).  Nothing is written at or beyond out + out_offset[nseg]. */
int64_t rdr_deflate_bound(int64_t n);
int rdr_deflate_encode(rdr_ctx* ctx, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                       void* out, int64_t out_capacity, int64_t* out_offset, int loc);
/* rdr_deflate_encode_tables: rdr_deflate_encode with a choice of tables - the same contract, errors and bound.  RDR_DEFL_FIXED is
 * rdr_deflate_encode, byte for byte.  RDR_DEFL_DYNAMIC: every sub-block is the smallest of a stored block, a fixed-Huffman block and a
 * dynamic-Huffman block (BTYPE 10) over the same tokens, chosen on the device from the tokens' symbol counts (ties: stored, then
 * fixed); the code lengths are optimal under RFC 1951's limits of 15 and 7 bits.  Any other `tables` is RDR_ERR_INVALID before the
 * device is touched.  block_counts (HOST, 3, may be NULL): the stored, fixed and dynamic sub-blocks of the call. */
#define RDR_DEFL_FIXED 0
#define RDR_DEFL_DYNAMIC 1
int rdr_deflate_encode_tables(rdr_ctx* ctx, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes,
                              int64_t nseg, int tables, void* out, int64_t out_capacity, int64_t* out_offset, int64_t* block_counts, int loc);
/* rdr_h5_chunks: a C-ordered array of `ndim` <= 4 axes (shape, HOST) of elem_bytes 1 / 2 / 4 / 8 cut into chunks (chunk, HOST) in
 * row-major chunk order.  Every chunk is full size: elements beyond the array's edge are `fill` (HOST, elem_bytes bytes).  shuffle:
 * each chunk is byte-transposed as HDF5's shuffle filter does, out[j * n + i] = in[i * elem_bytes + j] over the chunk's n elements.
 * out holds prod(ceil(shape / chunk)) * prod(chunk) elements; array and out live at `loc`. */
int rdr_h5_chunks(rdr_ctx* ctx, const void* array, int elem_bytes, int ndim, const int64_t* shape, const int64_t* chunk, const void* fill,
                  int shuffle, void* out, int loc);

/* ---- zlib streams decoded on the device (raider_amd/deflate.py, tifflite.py, h5lite.py) -------------------------------------------
 * rdr_inflate_decode: `nseg` independent zlib streams (RFC 1950 wrapper, RFC 1951 body) out of one byte buffer `src` of `src_bytes`:
 * stream i is src[seg_offset[i] .. + seg_bytes[i]), at any byte offset, and is written to out + i * out_stride, at most
 * seg_out_bytes[i] <= out_stride bytes of it.  status[i] is one of RDR_INFL_*; it is RDR_INFL_OK exactly when zlib 1.2.11's inflate
 * (as zlib.decompress drives it) accepts the stream and its output fits the slot, and then the slot's bytes are zlib's.  Bytes behind
 * the Adler-32 are ignored.  A bad stream sets its status and stops: nothing outside its segment is read, nothing outside
 * [slot, slot + seg_out_bytes[i]) is written, and slot bytes the stream does not reach keep their value.  produced[i] (may be NULL):
 * the bytes written to slot i.  src, out, status and produced live at `loc`; the three int64 tables are HOST arrays.  One wave per
 * stream, the 32 KiB history a ring in LDS from which the output is flushed: the output is never read back.  RDR_ERR_INVALID, before
 * the device is touched: NULL, src_bytes / nseg / out_stride <= 0, nseg > 2^24, a segment outside src or of 2 GiB or more, a slot
 * beyond out_stride, out_stride >= 2 GiB, nseg * out_stride > 2^40.  seg_bytes[i] == 0 is NOT an error of the call (as for
 * rdr_tiff_lzw_decode: a file may hold an empty segment beside good ones): that stream gets RDR_INFL_SHORT. */
#define RDR_INFL_OK 0        /* the final block ended, the Adler-32 matches, the output fits the slot */
#define RDR_INFL_SHORT 1     /* the input ended before the final block or its trailer */
#define RDR_INFL_OVERFLOW 2  /* the stream holds more than the slot takes */
#define RDR_INFL_INVALID 3   /* bad CMF / FLG, a preset dictionary, block type 3, LEN != ~NLEN, a bad code set or symbol, a distance too far back */
#define RDR_INFL_CHECKSUM 4  /* Adler-32 mismatch */
int rdr_inflate_decode(rdr_ctx* ctx, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, int64_t nseg,
                       const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int64_t* produced, int loc);
/* rdr_inflate_decode_split: rdr_inflate_decode with long streams decoded by many waves.  Arguments, locations and the RDR_ERR_INVALID
 * conditions (checked before the device is touched) are rdr_inflate_decode's, and for every stream, good or bad, status[i], produced[i]
 * and every byte of slot i are exactly what rdr_inflate_decode gives for the same arguments and the same pre-filled `out`.  pieces
 * (HOST, nseg, may be NULL): the pieces of stream i that separate waves decoded; 1: the stream went through the serial kernel.
 * A stream is cut where a byte-aligned empty stored block (00 00 FF FF: Z_SYNC_FLUSH, Z_FULL_FLUSH, the close of every 32 KiB
 * sub-block rdr_deflate_encode does not store) ends: of the marker occurrences that end in the same 1024-byte window of the stream
 * (window j = stream offsets [1024 j, 1024 j + 1024)) only the first and the last are candidates, so a stream of n bytes has at most
 * 2 (n / 1024 + 1).
 * A measure pass decodes every piece without output and records its length, where it ends and how far its matches reach behind its
 * start; a piece that reaches back is joined with its predecessors (Z_SYNC_FLUSH keeps the history), a false candidate is one no
 * piece ends on.  A stream whose chain of pieces is not provably clean - an error, no trailer, more output than the slot, a distance
 * too far back - is decoded by rdr_inflate_decode's kernel, which sets its status as ever.  The call ALWAYS synchronises with the
 * context's stream, twice on the way (the candidate counts and the measured pieces come to the host, where the plan is made), so
 * unlike rdr_inflate_decode it does not queue behind device work when loc is RDR_DEVICE.  (A piece that did not decode as it was
 * measured would give its stream RDR_INFL_INVALID: an internal-consistency status that no input can cause - both passes run the same
 * decoder over the same bytes - and the one outcome the equality with rdr_inflate_decode does not cover.) */
int rdr_inflate_decode_split(rdr_ctx* ctx, const void* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes,
                             int64_t nseg, const int64_t* seg_out_bytes, void* out, int64_t out_stride, int32_t* status, int64_t* produced,
                             int64_t* pieces, int loc);
/* rdr_h5_unchunk: the inverse of rdr_h5_chunks.  `npresent` decoded chunks, chunk k at chunks + k * chunk_stride and chunk_index[k]
 * (HOST) its row-major index in the chunk grid ceil(shape / chunk), each index at most once -> the C-ordered array out of `shape`.
 * Edge chunks are clipped, the shuffle is undone (`shuffle`), bytes are reversed within an element (`swap`); elements of chunks
 * that are not in the table are 0.  chunks and out live at `loc`; shape, chunk and chunk_index are HOST arrays.  RDR_ERR_INVALID:
 * NULL, elem_bytes / ndim / sizes out of range, more than 2^36 elements, npresent outside 1 .. the grid's chunk count, an index
 * outside the grid or given twice, chunk_stride below one chunk. */
int rdr_h5_unchunk(rdr_ctx* ctx, const void* chunks, int64_t chunk_stride, const int64_t* chunk_index, int64_t npresent, int elem_bytes, int ndim,
                   const int64_t* shape, const int64_t* chunk, int shuffle, int swap, void* out, int loc);

/* ---- exact all-pair empirical variograms of a station series (raider_amd/variogram.py; csrc/variogram_kernels.h) -------------------
 * The core of raiderStats (cli/statsPlot.py:573-659) over ALL n (n - 1) / 2 pairs of n points, where the reference samples 1000.
 * x, y [n]: metres.  values [nd][n]: one row per date, NaN = missing.  A pair i < j counts on a date when both its values are not
 * NaN; its lag is h = sqrt(dx * dx + dy * dy), evaluated without contraction (the value NumPy gets), its semivariance
 * g = 0.5 * (v_i - v_j)^2.
 * rdr_pair_distance_max: hmax[d] = the largest h over the pairs of date d, NaN for a date with fewer than two valid points (the
 * reference's default bins end at 0.67 of it, :638).
 * rdr_pair_variogram: edges [nedge_rows][nbins + 1], finite and strictly ascending, one row for all dates (nedge_rows = 1) or one
 * per date (nedge_rows = nd).  A pair goes to the bin b with edges[b] < h <= edges[b + 1] (:644); h <= edges[0] and h > edges[nbins]
 * are dropped.  count [nd][nbins] is exact; lag_sum and gamma_sum [nd][nbins] are f64 sums of h and g, added in an order that may
 * differ between calls (within (m - 1) * 2^-53 relative of the exact sum of a bin of m pairs); an empty bin gives 0, 0.0, 0.0.
 * Dates run in groups of at most four per launch, which share the pair distances.  No floating-point atomic touches global memory.
 * Every array lives at `loc`; a call with host outputs synchronises.  RDR_ERR_INVALID, before the device is touched and with the
 * outputs unwritten: NULL, a wrong loc, n outside 2 .. 2^20, nd outside 1 .. 4096, nbins outside 1 .. 64, nedge_rows not 1 or nd, an
 * edge row that is not finite or not strictly ascending (a row on the device is read back for this check). */
int rdr_pair_distance_max(rdr_ctx* ctx, const double* x, const double* y, int64_t n, const double* values, int nd, double* hmax, int loc);
int rdr_pair_variogram(rdr_ctx* ctx, const double* x, const double* y, int64_t n, const double* values, int nd, const double* edges, int nedge_rows,
                       int nbins, int64_t* count, double* lag_sum, double* gamma_sum, int loc);

/* rdr_cell_variogram: the all-pair variograms of EVERY grid cell and date in one pass (cli/statsPlot.py:721-814, _append_variogram
 * without its sampling; csrc/cell_variogram_kernels.h).  x, y [n], values [nd][n]: as above, the stations SORTED BY CELL - cell c owns
 * the stations cell_start[c] .. cell_start[c + 1] - 1 (cell_start [ncells + 1], ascending, first 0, last n; an empty cell is allowed).
 * Per slice (cell c, date d), over the pairs of the cell's stations valid on the date:
 *   nvalid [ncells][nd]   the valid stations;
 *   status [ncells][nd]   0 done; 1 skipped: nvalid < min_valid; 2 (deramp only) the plane is numerically singular - the determinant of
 *                         the centred 2 x 2 normal matrix is not above 1e-12 (Sxx + Syy)^2: fewer than three stations, stations at one
 *                         place or within 1e-6 of their extent of one line - and the slice is left to the caller's lstsq.  A slice with status != 0 has count 0, sums 0.0,
 *                         hmax NaN and, with deramp, NaN residuals;
 *   deramp = 1            the plane a x + b y + c fitted to the valid stations (centred normal equations, f64, a fixed summation order)
 *                         is removed before the pairs are formed; residuals (NULL or [nd][n], NaN where values is) receives the result.
 *                         residuals must not overlap values, and is refused without deramp;
 *   hmax [ncells][nd]     the largest h, NaN without a valid pair;
 *   edges = NULL          the reference's default row per slice, np.linspace(0, 0.67 * hmax, nbins + 1) bit for bit (:638);
 *   edges != NULL         [ncells][nbins + 1], one finite, strictly ascending row per cell, for all its dates;
 *   edges_out             NULL or [ncells][nd][nbins + 1]: the row of each slice (NaN for a default row without a pair);
 *   count, lag_sum, gamma_sum [ncells][nd][nbins]: as rdr_pair_variogram's, the same bin rule and the same bound on the sums;
 *   tot_count, tot_lag, tot_gamma  NULL (all three) or [ncells][nbins], given edges only: the slices of a cell with status 0 added in
 *                         date order - with all pairs kept, _binned_vario of the dates' concatenated raw arrays (:793-801).
 * One workgroup owns a (cell, group of 4 / 2 / 1 dates): three launches at most, no partials, no floating-point atomic on global memory,
 * counts identical between calls.  A cell of up to 512 stations is staged in LDS; a larger one runs from global memory in ONE
 * workgroup (no limit but n, and no speed to expect beyond some thousand stations per cell).  Every array lives at `loc`; with deramp
 * and residuals = NULL a work array of nd * n doubles is taken from the context.  RDR_ERR_INVALID, before any launch and with the outputs
 * unwritten: NULL (x, y, cell_start, values, nvalid, hmax, status, count, lag_sum, gamma_sum), a wrong loc, n outside 2 .. 2^20, nd
 * outside 1 .. 4096, nbins outside 1 .. 64, ncells outside 1 .. 2^20, min_valid < 0, deramp not 0 or 1, residuals without deramp, some
 * but not all of tot_*, totals without edges, cell_start not starting at 0, not ending at n or not ascending, an edge row that is not
 * finite or not strictly ascending (arrays on the device are read back for these checks). */
int rdr_cell_variogram(rdr_ctx* ctx, const double* x, const double* y, int64_t n, const int64_t* cell_start, int ncells, const double* values, int nd,
                       int deramp, int min_valid, const double* edges, int nbins, int64_t* nvalid, double* hmax, int32_t* status, int64_t* count,
                       double* lag_sum, double* gamma_sum, double* edges_out, double* residuals, int64_t* tot_count, double* tot_lag, double* tot_gamma,
                       int loc);

/* rdr_grid_stats: the gridded station statistics of raiderStats (cli/statsPlot.py create_DF, :1571-1794; csrc/grid_stats_kernels.h).
 * values [nd][n]: one row per date, NaN = no row, every other value - +-inf included - is a value; the stations SORTED BY CELL as for
 * rdr_cell_variogram (cell_start [ncells + 1], ascending, first 0, last n; an empty cell is allowed).
 * Per station [n]:
 *   st_nobs (int64)       its values;
 *   st_mean, st_median, st_stdev   over them; NaN without a value, st_stdev (ddof = 1) NaN below two.
 * Per cell [ncells], of its stations:
 *   nstations (int64)     the stations with a value;
 *   mean_of_means, mean_of_medians, mean_of_stdevs   the mean of the station statistic over the cell's stations where it is not NaN,
 *                         added in station order; NaN when none is left.
 * Per cell [ncells], over all values of its stations at once:
 *   cell_nobs (int64), abs_mean, abs_median, abs_stdev   as for a station.
 * A mean is sum / count, a deviation sqrt(sum of (v - mean)^2 / (count - 1)) in a second pass; f64, every sum in a fixed order: two
 * calls give the same bytes.  A median is (s[(m - 1) / 2] + s[m / 2]) / 2 of the m sorted values, bit for bit, found by exact radix
 * selection on the order-preserving 64-bit keys (-0 below +0), a byte per pass, without sorting.  No floating-point atomic at all.
 * Groups: (st_nobs, st_mean, st_stdev), (nstations, mean_of_means, mean_of_stdevs) and (cell_nobs, abs_mean, abs_stdev) are each given
 * whole or NULL whole - a NULL group is not computed unless another needs it (then in a work array of the context) -; each of the three
 * medians may be NULL on its own, which skips its selection, and is refused without its group.  A workgroup owns 64 stations, then one
 * owns a cell: a huge cell runs in ONE workgroup, with no speed to expect.  Every array lives at `loc`; a call with host outputs
 * synchronises.  RDR_ERR_INVALID, before any launch and with the outputs unwritten: NULL values or cell_start, a wrong loc, n outside
 * 1 .. 2^20, nd outside 1 .. 4096, ncells outside 1 .. 2^20, a partly NULL group, every group NULL, cell_start not starting at 0, not
 * ending at n or not ascending (an array on the device is read back for this), a cell of more than 2^31 - 1 slots (nd x its stations). */
int rdr_grid_stats(rdr_ctx* ctx, const double* values, int64_t n, int nd, const int64_t* cell_start, int ncells, int64_t* st_nobs, double* st_mean,
                   double* st_median, double* st_stdev, int64_t* nstations, double* mean_of_means, double* mean_of_medians, double* mean_of_stdevs,
                   int64_t* cell_nobs, double* abs_mean, double* abs_median, double* abs_stdev, int loc);

/* rdr_seasonal_fit: the seasonal sinusoids of raiderStats (cli/statsPlot.py _amplitude_and_phase, :2311-2479, and the cell means behind
 * the grid_seasonal_* maps, :1796-2309; csrc/seasonal_kernels.h).  Per station the exact least-squares fit of
 *     y ~ A sin(w t + p) + c      (linear in a = A cos p_c, b = A sin p_c, c at a given w; tau = t - t_ref, t_ref the middle of the axis)
 * to its values, at omega[0] (scan = 0: the reference's fixed period, k must be 1) or at the frequency of the band omega[0 .. k) where
 * the residual sum R(w) is smallest (scan = 1): k* = argmin over the grid (the lowest index on ties), then a golden-section search of R
 * inside [omega[k* - 1], omega[k* + 1]] (clipped to the band) until the bracket is below 1e-10 of omega[1] - omega[0], R is flat to
 * round-off, or 64 steps; the best frequency evaluated wins.  The reference's Levenberg-Marquardt run from one FFT bin ends in this
 * minimum often, not always; where it does not, this fit has the lower residual.
 *   t [nd]            HOST, whatever loc: POSIX seconds of the dates, finite, in any order.
 *   values [nd][n]    at loc: one row per date, NaN = no row; station-contiguous rows as for rdr_grid_stats.
 *   omega [k]         HOST: angular frequencies in rad / s, finite, > 0, ascending (scan: an evenly spaced grid is what makes sense).
 *   min_span, min_frac  the reference's eligibility (:2346-2347), evaluated on the device: a station is fitted when
 *                     span = (max t - min t of its rows) / 31556952 >= min_span, rows / (span * 365.25) >= min_frac and rows >= P + 1,
 *                     P = 3 parameters (scan = 0) or 4 (scan = 1).  (The reference accepts rows = P, with an infinite covariance.)
 *   cell_start [ncells + 1], cells   at loc, both or neither: the stations sorted by cell as for rdr_grid_stats.
 *   station [16][n]   at loc, doubles: 0 rows, 1 span in years, 2 fitted (0 / 1), 3 at_edge (k* is the first or last grid index),
 *                     4 A = hypot(a, b), 5 p in (-pi, pi] (for t in POSIX seconds), 6 c, 7 w, 8 R, 9 rmse = sqrt(R / (rows - 2)),
 *                     10 .. 13 the sigmas of A, w (NaN for scan = 0), p, c: square roots of the diagonal of R / (rows - P) (J^T J)^-1 with
 *                     the analytic Jacobian at the solution (formed with tau centred and in years, then carried to t), 14 k* (NaN for
 *                     scan = 0), 15 the golden-section steps taken.  A station that is not fitted - not eligible, a singular system,
 *                     a non-finite result - has 0 in rows 2 and 3 and NaN in rows 4 .. 15.
 *   cells [14][ncells]  per cell, over its fitted stations in station order: rows 0 .. 6 the plain means of the reference's columns
 *                     phsfit = 182.625 sin(p), ampfit, periodfit = 1 / (w / 2 pi * 31556952) years, phsfit_c, ampfit_c, periodfit_c,
 *                     seasonalfit_rmse, rows 7 .. 13 their means weighted by the stations' row counts (the reference's groupby over the
 *                     long table); NaN for a cell without a fitted station.  The three *_c columns carry the reference's labels
 *                     (:2424-2426: ampfit_c, periodfit_c, phsfit_c = sqrt of pcov[0,0], [1,1], [2,2]): for scan = 1 the sigmas of A, w, p,
 *                     for scan = 0 - parameters (A, p, c) - periodfit_c is the sigma of p and phsfit_c the sigma of c.
 * sin / cos of omega[k] tau[d] are computed once per (k, d); a lane owns a station and adds every sum in date order, f64, without any
 * floating-point atomic: two calls, host or device arrays, and any order of the stations give the same bytes per station.
 * A call with host outputs synchronises.  RDR_ERR_INVALID, before the device is touched: a NULL ctx, t, values, omega or station, a wrong
 * loc, n outside 1 .. 2^20, nd outside 1 .. 4096, k outside 1 .. 4096, scan not 0 / 1, scan = 0 with k != 1, min_span negative or not
 * finite, min_frac not finite, an omega that is not finite, not > 0 or not ascending, a t that is not finite, cell_start without cells or
 * the reverse, ncells outside 1 .. 2^20; and, after cell_start was read back from the device where it lives there: cell_start not
 * starting at 0, not ending at n or not ascending. */
int rdr_seasonal_fit(rdr_ctx* ctx, const double* t, const double* values, int64_t n, int nd, const double* omega, int k, int scan, double min_span,
                     double min_frac, const int64_t* cell_start, int ncells, double* station, double* cells, int loc);

/* rdr_variogram_fit: exponential variogram models (cli/statsPlot.py _fit_vario with __exponential__, nugget=False, :661-713;
 * csrc/variogram_fit_kernels.h) as EXACT BOUNDED MINIMA of the reference's own objective over the reference's own box - not the point at
 * which scipy's trust-region run happens to stop.  One fit per row f of h [nfits][m], gamma [nfits][m] (f64); a column where either is
 * NaN is absent; n is the number of columns present.
 *   model      b (1 - exp(-h / a)): range a, sill b.  The reference's third parameter never enters a model without nugget.
 *   bounds     0 <= a <= ub_a, 0 <= b <= ub_b: from ub [nfits][3] when given, else the reference's defaults
 *              0.8 * (max h, max gamma, max gamma) over the row's present columns.
 *   objective  scipy's cost for loss='soft_l1', f_scale = s:  C(a, b) = s^2 sum_i (sqrt(1 + z_i) - 1),  z_i = (r_i (1 / s))^2,
 *              r_i = b e_i - gamma_i,  e_i = 1 - exp(-h_i / a); each term evaluated as z_i / (sqrt(1 + z_i) + 1), which keeps its digits at
 *              z ~ 1e-6 (delays in metres), where the textbook form loses six.
 *   sill       for a given range C is convex in b and D(b) = sum e_i r_i / sqrt(1 + z_i) non-decreasing: D(0) >= 0 gives b = 0,
 *              D(ub_b) <= 0 gives b = ub_b, else bisection of [0, ub_b] (D > 0: the upper half is dropped) until the bracket is at most
 *              2^-52 ub_b wide or 64 halvings; b is the middle of the bracket.
 *   range      a_floor = h_pos / 38, h_pos the smallest positive present lag (exp(-38) < 2^-54: below it every e_i of a positive lag is
 *              exactly 1 and the model no longer depends on a).  k_scan candidates a_k = a_floor exp(k ln(ub_a / a_floor) / (k_scan - 1)),
 *              the first exactly a_floor, the last exactly ub_a (ub_a <= a_floor: the single candidate ub_a, no refinement); the
 *              candidate of lowest C, each at its own best sill, the lowest index on ties; then 8 rounds of 64 candidates spaced the same
 *              way over [a_(k-1), a_(k+1)] of the round before (clipped to its grid, end points included), each round centred on its
 *              own best.  The best candidate evaluated anywhere wins; a tie stays with the earlier round, then the lower index.
 *   outputs    params [nfits][3] = (a, b, ub_c / 2): the third is the reference's untouched nugget start; cost [nfits] = C(a, b);
 *              rmse [nfits] = sqrt(mean r_i^2), the reference's sqrt(nanmean(fun^2)); n [nfits] (int64);
 *              status [nfits] (int32), decided in this order: 1 no column present; 2 a negative lag or an infinity among the present
 *              values; 3 no positive lag (every e_i is 0); 2 ub_a or ub_b not finite or <= 0 (max gamma <= 0, where scipy raises);
 *              0 fitted.  A row with status != 0 holds NaN in params, cost and rmse and 0 in flags;
 *              flags [nfits] (int32) bits: 1 range at a_floor, 2 range at ub_a (within 2^-40 of the bound: the last round's candidates
 *              lie a few ulp apart), 4 sill 0, 8 sill ub_b (by the two tests on D).
 * One wave per row.  n <= 64: lanes are range candidates, e_i is kept per (point, lane) in LDS for the bisection, a lane adds its sums in
 * column order.  n > 64: lanes stride over the columns, candidates run one after the other, a sum is the lanes' partial sums folded by a
 * fixed butterfly.  The two may differ in round-off from each other; each is deterministic: a row's bytes depend on nothing but the row,
 * not on the batch, its position in it, the place of the arrays, or the run.  No floating-point atomic.
 * Every array lives at `loc`; a call with host outputs synchronises.  RDR_ERR_INVALID, before the device is touched: a NULL ctx, h,
 * gamma or output, a wrong loc, nfits outside 1 .. 2^22 (an empty batch is an error), m outside 1 .. 65536, nfits x m beyond 2^30,
 * f_scale not finite or <= 0, k_scan not a multiple of 64 in 64 .. 4096. */
int rdr_variogram_fit(rdr_ctx* ctx, const double* h, const double* gamma, int64_t nfits, int m, const double* ub, double f_scale, int k_scan,
                      double* params, double* cost, double* rmse, int64_t* n, int32_t* status, int32_t* flags, int loc);

#ifdef __cplusplus
}
#endif
#endif /* RAIDER_HIP_H */
