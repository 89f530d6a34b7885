//! `vit_tracker` over libvittrack_hip.so: the API the reference host links today
//! (`vit_tracker::{VitTrack, BBox}`, /root/reference/src/tracker_context.rs:2,
//! src/selection_state.rs:1), unchanged in names, argument meaning and error behaviour, so that
//! tracker_context.rs, selection_state.rs, pipeline*.rs and nv12_convert.rs compile as they are.
//!
//!   VitTrack::new(model_path)      src/tracker_context.rs:21     -> vt_create
//!   tracker.init(&view, bbox)      src/tracker_context.rs:88     -> vt_init_rgb8   (result ignored by the host)
//!   tracker.update(&view)          src/tracker_context.rs:90,120 -> vt_update_rgb8
//!   BBox::new / BBox::from_array   src/selection_state.rs:44, src/tracker_context.rs:94
//!
//! Nothing unwinds across the C boundary (the host is built with panic = "abort", Cargo.toml:37):
//! every C entry returns a status code, surfaced here as `Err(TrackError)`. For the same reason this
//! file contains no `assert!`, `unwrap()`, `expect(` or `panic!` and no slice indexing that can fail
//! (tests/test_rust_binding.py greps for them): a view the library cannot take is an `Err` from
//! `update`; `init`, whose result the host discards (src/tracker_context.rs:88), records the error and
//! the next `update` returns it.
pub mod sys;

use ndarray::ArrayView3;
use std::ffi::{c_int, c_void, CStr, CString};

pub use sys::BBox;
/// The colour meaning of a YUV frame (BT.601 / BT.709 / BT.2020, limited / full range) and the `const fn` that forms
/// `VtFrame::format` from a pixel format and the two: a plain pixel format value stays BT.601 limited range.
pub use sys::{vt_frame_format as frame_format, VT_COLOR_BT2020, VT_COLOR_BT601, VT_COLOR_BT709, VT_RANGE_FULL, VT_RANGE_LIMITED};

impl BBox {
    /// src/selection_state.rs:44
    pub fn new(x: i32, y: i32, width: i32, height: i32) -> Self {
        Self { x, y, width, height }
    }
    /// src/tracker_context.rs:94,123
    pub fn from_array(a: &[i32; 4]) -> Self {
        Self::new(a[0], a[1], a[2], a[3])
    }
}

/// Error of a library call: the vt_status code and vt_last_error()'s text. `Debug` is what the host
/// prints (`{:?}`, src/tracker_context.rs:22,106,135).
#[derive(Debug, Clone)]
pub struct TrackError {
    pub code: i32,
    pub text: String,
}
impl std::fmt::Display for TrackError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "vittrack_hip error {}: {}", self.code, self.text)
    }
}
impl std::error::Error for TrackError {}

fn last(code: c_int) -> TrackError {
    let text = unsafe { CStr::from_ptr(sys::vt_last_error()) }.to_string_lossy().into_owned();
    TrackError { code, text }
}

/// What `update` returns: the fields the host reads at src/tracker_context.rs:92-95,122-125.
#[derive(Debug, Clone, Copy)]
pub struct TrackResult {
    pub success: bool,
    pub score: f32,
    pub bbox: [i32; 4],
}
impl From<sys::VtResult> for TrackResult {
    fn from(r: sys::VtResult) -> Self {
        Self { success: r.success != 0, score: r.score, bbox: [r.bbox.x, r.bbox.y, r.bbox.width, r.bbox.height] }
    }
}

pub struct VitTrack {
    h: *mut sys::vt_tracker,
    /// an `init` that failed (the host ignores init's result): returned by the next `update`
    pending: Option<TrackError>,
}
// Constructed on the main thread (src/main.rs:49 -> src/pipeline_ir.rs:89), used only on the GStreamer
// streaming thread behind a Mutex (src/pipeline.rs:55-67,110-119). The C handle has no thread affinity
// (every entry point selects and restores the HIP device): tests/test_gpu_threading.py.
unsafe impl Send for VitTrack {}

impl VitTrack {
    /// ≙ src/tracker_context.rs:21. `model_path` is a VTWB0001 weight blob; the device comes from
    /// VITTRACK_DEVICE (default 0).
    pub fn new(model_path: &str) -> Result<Self, TrackError> {
        let dev = std::env::var("VITTRACK_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
        Self::with_device(model_path, dev)
    }

    pub fn with_device(model_path: &str, device: i32) -> Result<Self, TrackError> {
        let p = CString::new(model_path).map_err(|_| TrackError { code: sys::VT_ERR_INVALID_ARG, text: "path has NUL".into() })?;
        let mut cfg = std::mem::MaybeUninit::<sys::VtConfig>::uninit();
        let mut h = std::ptr::null_mut();
        let rc = unsafe {
            sys::vt_config_default(cfg.as_mut_ptr());
            sys::vt_create(p.as_ptr(), device, cfg.as_ptr(), &mut h)
        };
        if rc != sys::VT_OK {
            Err(last(rc))
        } else {
            Ok(Self { h, pending: None })
        }
    }

    /// The (H, W, 3) RGB8 views the host builds (src/nv12_convert.rs:90, src/pipeline_ir.rs:142) have strides
    /// (W*3, 3, 1); rows may be padded. Anything else is VT_ERR_INVALID_ARG - never a panic (panic = "abort").
    fn rgb_view(img: &ArrayView3<u8>) -> Result<(*const u8, c_int, c_int, c_int), TrackError> {
        let (h, w, c) = img.dim();
        let bad = |text: &str| TrackError { code: sys::VT_ERR_INVALID_ARG, text: text.into() };
        let (s0, s1, s2) = match img.strides() {
            [a, b, c] => (*a, *b, *c),
            _ => return Err(bad("3-dimensional view expected")),
        };
        if c != 3 || s2 != 1 || s1 != 3 || s0 < 3 * w as isize {
            return Err(bad("RGB8 HWC view with strides (>= W*3, 3, 1) expected"));
        }
        if w > c_int::MAX as usize || h > c_int::MAX as usize || s0 > c_int::MAX as isize {
            return Err(bad("view too large"));
        }
        Ok((img.as_ptr(), w as c_int, h as c_int, s0 as c_int))
    }

    /// ≙ src/tracker_context.rs:88 (the host discards the result; `()` keeps its code unchanged). A failure is kept
    /// and returned by the next `update` (which the host calls on the same frame, :90).
    pub fn init(&mut self, img: &ArrayView3<u8>, bbox: BBox) {
        self.pending = match Self::rgb_view(img) {
            Err(e) => Some(e),
            Ok((p, w, h, s)) => {
                let rc = unsafe { sys::vt_init_rgb8(self.h, p, w, h, s, bbox) };
                if rc != sys::VT_OK { Some(last(rc)) } else { None }
            }
        };
    }

    /// ≙ src/tracker_context.rs:90,120
    pub fn update(&mut self, img: &ArrayView3<u8>) -> Result<TrackResult, TrackError> {
        if let Some(e) = self.pending.take() {
            return Err(e);
        }
        let (p, w, h, s) = Self::rgb_view(img)?;
        let mut r = sys::VtResult::default();
        let rc = unsafe { sys::vt_update_rgb8(self.h, p, w, h, s, &mut r) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(r.into())
    }

    /// (Y plane, UV plane) of a packed NV12 buffer, or VT_ERR_SHORT_BUFFER / VT_ERR_INVALID_ARG - no indexing that can panic
    fn nv12_planes(nv12: &[u8], w: usize, h: usize) -> Result<(*const u8, *const u8, c_int, c_int), TrackError> {
        let px = w.checked_mul(h).filter(|_| w <= c_int::MAX as usize && h <= c_int::MAX as usize);
        let px = px.ok_or(TrackError { code: sys::VT_ERR_INVALID_ARG, text: "frame size out of range".into() })?;
        let uv = nv12.get(px..).filter(|uv| uv.len() >= px / 2);
        let uv = uv.ok_or(TrackError { code: sys::VT_ERR_SHORT_BUFFER, text: "nv12 buffer shorter than w*h*3/2".into() })?;
        Ok((nv12.as_ptr(), uv.as_ptr(), w as c_int, h as c_int))
    }

    /// Fused NV12 ingest (not in the original crate): the same result as init/update on the RGB frame
    /// nv12_full_to_rgb_parallel (src/nv12_convert.rs:46) would have produced, without converting the
    /// whole frame; lets src/pipeline.rs:104-106 go. `nv12` is the mapped buffer (Y plane then
    /// interleaved UV, stride == width as src/nv12_convert.rs:53-54 assumes).
    pub fn init_nv12(&mut self, nv12: &[u8], w: usize, h: usize, bbox: BBox) {
        self.pending = match Self::nv12_planes(nv12, w, h) {
            Err(e) => Some(e),
            Ok((y, uv, wi, hi)) => {
                let rc = unsafe { sys::vt_init_nv12(self.h, y, uv, wi, hi, wi, wi, bbox) };
                if rc != sys::VT_OK { Some(last(rc)) } else { None }
            }
        };
    }

    pub fn update_nv12(&mut self, nv12: &[u8], w: usize, h: usize) -> Result<TrackResult, TrackError> {
        if let Some(e) = self.pending.take() {
            return Err(e);
        }
        let (y, uv, wi, hi) = Self::nv12_planes(nv12, w, h)?;
        let mut r = sys::VtResult::default();
        let rc = unsafe { sys::vt_update_nv12(self.h, y, uv, wi, hi, wi, wi, &mut r) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(r.into())
    }

    /// Fused YUY2 ingest: the capture format of the live IR pipeline (src/pipeline_ir.rs:27-41)
    pub fn update_yuy2(&mut self, yuy2: &[u8], w: usize, h: usize) -> Result<TrackResult, TrackError> {
        if let Some(e) = self.pending.take() {
            return Err(e);
        }
        let need = w.checked_mul(h).and_then(|p| p.checked_mul(2)).filter(|_| w <= (c_int::MAX / 2) as usize && h <= c_int::MAX as usize);
        match need {
            None => return Err(TrackError { code: sys::VT_ERR_INVALID_ARG, text: "frame size out of range".into() }),
            Some(n) if yuy2.len() < n => return Err(TrackError { code: sys::VT_ERR_SHORT_BUFFER, text: "yuy2 buffer shorter than w*h*2".into() }),
            Some(_) => {}
        }
        let mut r = sys::VtResult::default();
        let rc = unsafe { sys::vt_update_yuy2(self.h, yuy2.as_ptr(), w as c_int, h as c_int, (2 * w) as c_int, &mut r) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(r.into())
    }

    pub fn model_info(&self) -> Result<sys::VtModelInfo, TrackError> {
        let mut mi = sys::VtModelInfo::default();
        let rc = unsafe { sys::vt_get_model_info(self.h, &mut mi) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(mi)
    }

    /// Let the device re-cut the template every `period` updates (0: off, else 2..=1_000_000) whose result succeeds with
    /// `score >= min_score` (vt_set_template_refresh): what a re-`init` with that update's frame and box would write,
    /// without leaving the update path. For a camera that tracks one target for hours.
    pub fn set_template_refresh(&mut self, period: i32, min_score: f32) -> Result<(), TrackError> {
        let rc = unsafe { sys::vt_set_template_refresh(self.h, period, min_score) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(())
    }

    /// Let the device cut a target chip of side `size` (a multiple of 8, 32..=512) behind every due update
    /// (vt_enable_chip): `kind` is sys::VT_CHIP_NORM_BF16 (planar [3][size][size] bf16 of v * norm_a[c] + norm_b[c]) or
    /// sys::VT_CHIP_RGB8 (packed [size][size][3] bytes; the norms are ignored). Fixed by the first call.
    pub fn enable_chip(&mut self, size: i32, kind: i32, norm_a: &[f32; 3], norm_b: &[f32; 3]) -> Result<(), TrackError> {
        let rc = unsafe { sys::vt_enable_chip(self.h, size, kind, norm_a.as_ptr(), norm_b.as_ptr()) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(())
    }

    /// The chip policy (vt_set_chip): `factor` 0 switches chips off, else (0.5..=4) the crop side is factor * sqrt(w * h)
    /// of the new box; a chip is cut after every update whose frames_done % period == phase.
    pub fn set_chip(&mut self, factor: f32, period: i32, phase: i32) -> Result<(), TrackError> {
        let rc = unsafe { sys::vt_set_chip(self.h, factor, period, phase) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(())
    }

    /// The chip as the last update left it, into `out` (at least 6 * size * size bytes for the bf16 kind, 3 * size * size
    /// for RGB8: a shorter buffer is refused here, the library cannot see its length), and its info (vt_read_chip). The
    /// bytes are current only where info.status == 1.
    pub fn read_chip(&mut self, size: i32, kind: i32, out: &mut [u8]) -> Result<sys::VtChipInfo, TrackError> {
        let per = if kind == sys::VT_CHIP_NORM_BF16 { 6usize } else { 3usize };
        let need = (size.max(0) as usize).saturating_mul(size.max(0) as usize).saturating_mul(per);
        if out.len() < need {
            return Err(bad("chip buffer too short"));
        }
        let mut info = sys::VtChipInfo::default();
        let rc = unsafe { sys::vt_read_chip(self.h, out.as_mut_ptr() as *mut c_void, &mut info) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(info)
    }

    /// The response-peaks policy (vt_set_peaks): `max_peaks` 0 switches the list off, else (1..=8) every update lists up to
    /// that many maxima of the score map with their decoded boxes, each suppressing the square of `radius` (1..=4) cells
    /// around it; a peak behind the first needs a response of at least `min_resp` (0..=1).
    pub fn set_peaks(&mut self, max_peaks: i32, radius: i32, min_resp: f32) -> Result<(), TrackError> {
        let rc = unsafe { sys::vt_set_peaks(self.h, max_peaks, radius, min_resp) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(())
    }

    /// The peaks of the last update (vt_last_peaks): peak 0 is the update's own box; a close runner-up says how near the
    /// call was. A peak's box can be handed to a candidate slot as it is.
    pub fn last_peaks(&mut self) -> Result<sys::VtPeaks, TrackError> {
        let mut p = sys::VtPeaks::default();
        let rc = unsafe { sys::vt_last_peaks(self.h, &mut p) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(p)
    }

    pub fn template_refresh_stats(&mut self) -> Result<sys::VtRefreshStats, TrackError> {
        let mut st = sys::VtRefreshStats::default();
        let rc = unsafe { sys::vt_template_refresh_stats(self.h, &mut st) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        Ok(st)
    }

    /// This tracker's stream as a snapshot (vt_export_state): state, refresh policy and the current template rows, one
    /// self-contained byte string. A later `VitTrack` of the same input geometry - another process, another GPU, another
    /// checkpoint - continues the track from it with `import_state`, without the operator selecting again.
    pub fn export_state(&self) -> Result<Vec<u8>, TrackError> {
        let mut need: usize = 0;
        let rc = unsafe { sys::vt_export_state(self.h, std::ptr::null_mut(), 0, &mut need) };
        if rc != sys::VT_ERR_SHORT_BUFFER {
            return Err(last(rc));
        }
        let mut buf = vec![0u8; need];
        let mut written: usize = 0;
        let rc = unsafe { sys::vt_export_state(self.h, buf.as_mut_ptr() as *mut c_void, buf.len(), &mut written) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        buf.truncate(written);
        Ok(buf)
    }

    /// Become the stream `snapshot` was exported from (vt_import_state). A snapshot that is malformed or of another
    /// input geometry is an `Err` (VT_ERR_FORMAT) and changes nothing.
    pub fn import_state(&mut self, snapshot: &[u8]) -> Result<(), TrackError> {
        let rc = unsafe { sys::vt_import_state(self.h, snapshot.as_ptr() as *const c_void, snapshot.len()) };
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        self.pending = None;
        Ok(())
    }
}

impl Drop for VitTrack {
    fn drop(&mut self) {
        unsafe { sys::vt_destroy(self.h) }
    }
}

/// ≙ nv12_full_to_rgb_parallel (src/nv12_convert.rs:46-92) on the GPU, bit for bit (including the
/// all-zero frame for a short buffer, :48-50); for callers that still want the whole RGB frame.
pub fn nv12_full_to_rgb(nv12: &[u8], w: usize, h: usize, device: i32) -> Result<Vec<u8>, TrackError> {
    let bytes = w.checked_mul(h).and_then(|p| p.checked_mul(3)).filter(|_| w <= c_int::MAX as usize && h <= c_int::MAX as usize);
    let bytes = bytes.ok_or(TrackError { code: sys::VT_ERR_INVALID_ARG, text: "frame size out of range".into() })?;
    let mut out = vec![0u8; bytes];
    let rc = unsafe { sys::vt_nv12_to_rgb8(device, nv12.as_ptr(), nv12.len(), w as c_int, h as c_int, out.as_mut_ptr()) };
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(out)
}

/// The pipelined subset pass of a group (vt_group_enqueue_host_streams): `host_frames[i]` feeds `streams[i]`; collect
/// with `sys::vt_group_wait_next`. A multi-camera host calls this for the cameras that are tracking this frame
/// (src/tracker_context.rs:90,120) while the previous frame's pass is still running.
///
/// # Safety
/// `g` is a live group handle; the planes of `host_frames` stay valid and unchanged until the pass is collected.
pub unsafe fn group_enqueue_host_streams(g: *mut sys::vt_group, streams: &[i32], host_frames: &[sys::VtFrame]) -> Result<(), TrackError> {
    if streams.len() != host_frames.len() || streams.len() > c_int::MAX as usize {
        return Err(TrackError { code: sys::VT_ERR_INVALID_ARG, text: "one frame per listed stream expected".into() });
    }
    let rc = sys::vt_group_enqueue_host_streams(g, streams.as_ptr(), host_frames.as_ptr(), streams.len() as c_int);
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(())
}

/// ≙ tracker.init (src/tracker_context.rs:88) on one camera of a group while the others keep tracking
/// (vt_group_enqueue_init_host): queued behind the outstanding pipelined passes, no wait for them.
///
/// # Safety
/// `g` is a live group handle; `host_frame`'s planes are readable for the duration of the call.
pub unsafe fn group_enqueue_init_host(g: *mut sys::vt_group, stream: i32, host_frame: &sys::VtFrame, bbox: BBox) -> Result<(), TrackError> {
    let rc = sys::vt_group_enqueue_init_host(g, stream, host_frame, bbox);
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(())
}

/// The candidate state boxes whose search windows tile a `w` x `h` frame (vt_scan_windows), row by row; needs no GPU.
/// Empty on arguments the library refuses.
pub fn scan_windows(w: i32, h: i32, box_w: f32, box_h: f32, overlap_pct: i32) -> Vec<[f32; 4]> {
    let n = unsafe { sys::vt_scan_windows(w, h, box_w, box_h, overlap_pct, std::ptr::null_mut(), 0) };
    if n <= 0 {
        return Vec::new();
    }
    let mut out = vec![[0f32; 4]; n as usize];
    let got = unsafe { sys::vt_scan_windows(w, h, box_w, box_h, overlap_pct, out.as_mut_ptr() as *mut f32, n) };
    out.truncate(got.clamp(0, n) as usize);
    out
}

/// Look for a lost camera's target over the whole frame instead of sitting the frame out (≙ the `Lost` branch of
/// src/tracker_context.rs:142-153): the windows of `scan_windows` for a `box_w` x `box_h` target, in grid order, in
/// candidate passes (vt_group_update_host_candidates) of as many slots as the group has streams. Stops at the first
/// pass whose winner succeeds and returns it, else the last pass's winner. Each pass is one update of `stream`; a
/// failed scan leaves the stream's box where it was.
///
/// # Safety
/// `g` is a live group handle with no pipelined pass outstanding; `host_frame`'s planes are readable for the
/// duration of the call.
pub unsafe fn group_reacquire_host(g: *mut sys::vt_group, stream: i32, host_frame: &sys::VtFrame, box_w: f32, box_h: f32,
                                   overlap_pct: i32) -> Result<TrackResult, TrackError> {
    let bad = |text: &str| TrackError { code: sys::VT_ERR_INVALID_ARG, text: text.into() };
    let slots = sys::vt_group_streams(g);
    if slots < 1 {
        return Err(bad("null group"));
    }
    let boxes = scan_windows(host_frame.width, host_frame.height, box_w, box_h, overlap_pct);
    if boxes.is_empty() {
        return Err(bad("scan_windows refused the frame or box size"));
    }
    let mut best: Option<TrackResult> = None;
    for chunk in boxes.chunks(slots as usize) {
        let cands: Vec<sys::VtCandidate> = chunk.iter().map(|b| sys::VtCandidate { stream, has_box: 1, r#box: *b }).collect();
        let frames: Vec<sys::VtFrame> = chunk.iter().map(|_| *host_frame).collect();
        let mut out = vec![sys::VtResult::default(); chunk.len()];
        let mut winner = vec![0i32; chunk.len()];
        let rc = sys::vt_group_update_host_candidates(g, cands.as_ptr(), frames.as_ptr(), chunk.len() as c_int, out.as_mut_ptr(),
                                                      winner.as_mut_ptr());
        if rc != sys::VT_OK {
            return Err(last(rc));
        }
        // every slot works for `stream`: winner[0] is the pass's winning slot
        let w = winner.first().copied().unwrap_or(0).max(0) as usize;
        let r: TrackResult = out.get(w).copied().ok_or_else(|| bad("winner out of range"))?.into();
        best = Some(r);
        if r.success {
            break;
        }
    }
    best.ok_or_else(|| bad("no scan window"))
}

/// The refresh policy of one camera of a group, or of all with `stream = -1` (vt_group_set_template_refresh): the
/// device re-cuts the template inside the pass, so the pipelined passes keep running full. Refused while a pipelined
/// pass is outstanding.
///
/// # Safety
/// `g` is a live group handle.
pub unsafe fn group_set_template_refresh(g: *mut sys::vt_group, stream: i32, period: i32, min_score: f32) -> Result<(), TrackError> {
    let rc = sys::vt_group_set_template_refresh(g, stream, period, min_score);
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(())
}

/// The chip policy of one camera of a group, or of all with `stream = -1` (vt_group_set_chips), after
/// sys::vt_group_enable_chips. Refused while a pipelined pass is outstanding.
///
/// # Safety
/// `g` is a live group handle.
pub unsafe fn group_set_chips(g: *mut sys::vt_group, stream: i32, factor: f32, period: i32, phase: i32) -> Result<(), TrackError> {
    let rc = sys::vt_group_set_chips(g, stream, factor, period, phase);
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(())
}

/// The response-peaks policy of one camera of a group, or of all with `stream = -1` (vt_group_set_peaks). The first call
/// with `max_peaks > 0` makes the engine peaks-capable. Refused while a pipelined pass is outstanding.
///
/// # Safety
/// `g` is a live group handle.
pub unsafe fn group_set_peaks(g: *mut sys::vt_group, stream: i32, max_peaks: i32, radius: i32, min_resp: f32) -> Result<(), TrackError> {
    let rc = sys::vt_group_set_peaks(g, stream, max_peaks, radius, min_resp);
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(())
}

/// The peak records of the last collected pass, one per slot in the pass's order, into `out` (vt_group_last_peaks).
///
/// # Safety
/// `g` is a live group handle.
pub unsafe fn group_last_peaks(g: *mut sys::vt_group, out: &mut [sys::VtPeaks]) -> Result<(), TrackError> {
    let n = i32::try_from(out.len()).unwrap_or(i32::MAX);
    let rc = sys::vt_group_last_peaks(g, out.as_mut_ptr(), n);
    if rc != sys::VT_OK {
        return Err(last(rc));
    }
    Ok(())
}
