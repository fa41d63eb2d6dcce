//! The reference's engine API (src/lib.rs:28-94) on the GPU, signatures unchanged:
//!
//! ```text
//! DistanceEngine::new(query: &EncodedBits) -> Self                               src/lib.rs:33
//! DistanceEngine::batch_process(&self, out: &mut [[u16; 31]], db: &[EncodedBits]) src/lib.rs:42
//! MasksEngine::new(query: &Bits) -> Self                                         src/lib.rs:60
//! MasksEngine::batch_process(&self, out: &mut [[u16; 31]], db: &[Bits])          src/lib.rs:69
//! distances(&EncodedBits, &EncodedBits) -> [u16; 31]                             src/lib.rs:82
//! denominators(&Bits, &Bits) -> [u16; 31]                                        src/lib.rs:89
//! ```
//!
//! With the `hip` feature, `src/lib.rs` re-exports these instead of its rayon engines
//!.  `new` builds the 31 rotated query copies once — on the device,
//! in the layouts the kernels read — as the reference builds them once on the host.
//! `batch_process` keeps the reference contract: host slices in, host `[u16; 31]`
//! rows out, blocking, `assert_eq!(out.len(), db.len())`.  The device-resident forms
//! (`*_resident`, `TemplateEngine::search`) are what a participant / resolver uses
//! once its share or masks file is loaded into a `Database`.
use std::ptr;

use super::{check, default_device, ffi, match_to_pair, Database, Device, Record, Result, ShardedDatabase};
use crate::{Bits, EncodedBits, Template};

/// The result of `TemplateEngine::report`, `MasksEngine::report` and `resolver_report`: the parts that were asked for, each as its sibling method
/// returns it.
#[derive(Clone, Debug, Default)]
pub struct Report {
    pub matches: Option<(Vec<(f64, usize)>, u64)>,
    pub topk: Option<Vec<(f64, usize)>>,
    pub histogram: Option<(Vec<u64>, u64)>,
}

/// Runs one `iris_*_matches` call: `call(out, cap, count)`.  `cap = None` returns every match (room
/// for 1024 first, then once more with room for the reported count); `Some(0)` only counts.
/// -> (the matches of lowest index as `(distance, index)`, ascending; the total count).
fn collect_matches(
    cap: Option<u64>,
    mut call: impl FnMut(*mut ffi::IrisMatch, u64, *mut u64) -> i32,
) -> Result<(Vec<(f64, usize)>, u64)> {
    let mut room = cap.unwrap_or(1024);
    let mut count = 0u64;
    let mut buf = vec![ffi::IrisMatch::default(); room as usize];
    check(call(if room == 0 { ptr::null_mut() } else { buf.as_mut_ptr() }, room, &mut count))?;
    if cap.is_none() && count > room {
        room = count;
        buf = vec![ffi::IrisMatch::default(); room as usize];
        check(call(buf.as_mut_ptr(), room, &mut count))?;
    }
    buf.truncate(count.min(room) as usize);
    Ok((buf.iter().map(match_to_pair).collect(), count))
}

/// Runs one `iris_*_topk` call: `call(out, count)` on a k-entry array -> the listed records as
/// `(distance, index)`, best first.
fn collect_topk(k: u32, mut call: impl FnMut(*mut ffi::IrisMatch, *mut u32) -> i32) -> Result<Vec<(f64, usize)>> {
    let mut count = 0u32;
    let mut buf = vec![ffi::IrisMatch::default(); k.max(1) as usize];
    check(call(buf.as_mut_ptr(), &mut count))?;
    buf.truncate(count as usize);
    Ok(buf.iter().map(match_to_pair).collect())
}

/// The k closest rows of the resolver's aggregation over device arrays of n * 31 u16, best first
/// (iris_resolver_topk; k = 1..=ffi::IRIS_TOPK_MAX has no reference counterpart).
pub fn resolver_topk(
    dev: &Device,
    shares_device: &[*const u16],
    denoms_device: *const u16,
    n: u64,
    index_base: u64,
    k: u32,
) -> Result<Vec<(f64, usize)>> {
    collect_topk(k, |out, count| unsafe {
        ffi::iris_resolver_topk(
            dev.raw(),
            shares_device.as_ptr(),
            shares_device.len() as u32,
            denoms_device,
            n,
            index_base,
            k,
            out,
            count,
        )
    })
}

/// The distance distribution of the resolver's aggregation over device arrays of n * 31 u16
/// (iris_resolver_histogram; no reference counterpart) -> (bins, invalid): a row is counted in bin
/// min(nbins - 1, floor(distance * nbins)), one without a valid rotation in `invalid` alone.
/// `nbins` is a power of two up to `ffi::IRIS_HIST_MAX_BINS`; histograms of chunks add.
pub fn resolver_histogram(
    dev: &Device,
    shares_device: &[*const u16],
    denoms_device: *const u16,
    n: u64,
    nbins: u32,
) -> Result<(Vec<u64>, u64)> {
    let mut bins = vec![0u64; nbins.clamp(1, ffi::IRIS_HIST_MAX_BINS) as usize];
    let mut invalid = 0u64;
    check(unsafe {
        ffi::iris_resolver_histogram(
            dev.raw(),
            shares_device.as_ptr(),
            shares_device.len() as u32,
            denoms_device,
            n,
            nbins,
            bins.as_mut_ptr(),
            &mut invalid,
        )
    })?;
    Ok((bins, invalid))
}

/// Runs one report call (iris_template_report, iris_resolver_report, iris_resolver_report_masks):
/// `call(report)` on an `IrisReport` filled from the selected parts -- `matches = Some((threshold,
/// cap))`, `k = Some(k)`, `nbins = Some(nbins)` -- -> the parts that were asked for.
fn collect_report(
    matches: Option<(f64, u64)>,
    k: Option<u32>,
    nbins: Option<u32>,
    mut call: impl FnMut(&mut ffi::IrisReport) -> i32,
) -> Result<Report> {
    let mut list = vec![ffi::IrisMatch::default(); matches.map_or(0, |m| m.1) as usize];
    let mut best = vec![ffi::IrisMatch::default(); k.map_or(0, |k| k.max(1)) as usize];
    let mut bins = vec![0u64; nbins.map_or(0, |b| b.clamp(1, ffi::IRIS_HIST_MAX_BINS)) as usize];
    let mut r = ffi::IrisReport {
        parts: 0,
        k: k.unwrap_or(0),
        nbins: nbins.unwrap_or(0),
        topk_count: 0,
        threshold: matches.map_or(0.0, |m| m.0),
        matches: if list.is_empty() { ptr::null_mut() } else { list.as_mut_ptr() },
        matches_cap: list.len() as u64,
        matches_count: 0,
        topk: best.as_mut_ptr(),
        bins: bins.as_mut_ptr(),
        invalid: 0,
    };
    if matches.is_some() {
        r.parts |= ffi::IRIS_REPORT_MATCHES;
    }
    if k.is_some() {
        r.parts |= ffi::IRIS_REPORT_TOPK;
    }
    if nbins.is_some() {
        r.parts |= ffi::IRIS_REPORT_HIST;
    }
    check(call(&mut r))?;
    list.truncate(r.matches_count.min(r.matches_cap) as usize);
    best.truncate(r.topk_count as usize);
    Ok(Report {
        matches: matches.map(|_| (list.iter().map(match_to_pair).collect(), r.matches_count)),
        topk: k.map(|_| best.iter().map(match_to_pair).collect()),
        histogram: nbins.map(|_| (bins, r.invalid)),
    })
}

/// Several of the resolver's matches, top-k and histogram over device arrays of n * 31 u16 from
/// ONE read of the share rows (iris_resolver_report; no reference counterpart).  Parts as in
/// `TemplateEngine::report`; each selected part is exactly what the sibling call returns.
pub fn resolver_report(
    dev: &Device,
    shares_device: &[*const u16],
    denoms_device: *const u16,
    n: u64,
    index_base: u64,
    matches: Option<(f64, u64)>,
    k: Option<u32>,
    nbins: Option<u32>,
) -> Result<Report> {
    collect_report(matches, k, nbins, |r| unsafe {
        ffi::iris_resolver_report(
            dev.raw(),
            shares_device.as_ptr(),
            shares_device.len() as u32,
            denoms_device,
            n,
            index_base,
            r as *mut ffi::IrisReport as *mut _,
        )
    })
}

/// An engine handle plus the device it lives on (kept alive by the clone).
struct Handle {
    raw: *mut ffi::IrisEngine,
    _device: Device,
}

unsafe impl Send for Handle {}
unsafe impl Sync for Handle {}

impl Drop for Handle {
    fn drop(&mut self) {
        unsafe {
            ffi::iris_engine_destroy(self.raw);
        }
    }
}

impl Handle {
    fn batch_process_host<T: Record>(&self, what: &str, out: &mut [[u16; 31]], db: &[T]) {
        assert_eq!(out.len(), db.len());
        if db.is_empty() {
            return;
        }
        check(unsafe {
            ffi::iris_engine_batch_process_host(self.raw, db.as_ptr().cast(), db.len() as u64, out.as_mut_ptr().cast())
        })
        .unwrap_or_else(|e| panic!("{what}::batch_process: {e}"));
    }

    fn batch_process_resident(&self, out: &mut [[u16; 31]], db: &Database, first: u64) -> Result<()> {
        check(unsafe {
            ffi::iris_engine_batch_process(self.raw, db.raw(), first, out.len() as u64, out.as_mut_ptr().cast())
        })
    }
}

/// `DistanceEngine` (src/lib.rs:28-53): out[i][k] = dot_u16(rot(query, k - 15), db[i]) mod 2^16.
pub struct DistanceEngine {
    h: Handle,
}

impl DistanceEngine {
    pub fn new(query: &EncodedBits) -> Self {
        Self::new_on(default_device(), query).unwrap_or_else(|e| panic!("DistanceEngine::new: {e}"))
    }

    pub fn new_on(device: &Device, query: &EncodedBits) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::iris_distance_engine_new(device.raw(), query.0.as_ptr(), &mut raw) })?;
        Ok(Self { h: Handle { raw, _device: device.clone() } })
    }

    pub fn batch_process(&self, out: &mut [[u16; 31]], db: &[EncodedBits]) {
        self.h.batch_process_host("DistanceEngine", out, db)
    }

    /// Records [first, first + out.len()) of a resident share database.
    pub fn batch_process_resident(&self, out: &mut [[u16; 31]], db: &Database, first: u64) -> Result<()> {
        self.h.batch_process_resident(out, db, first)
    }
}

/// `nq` DistanceEngines at once (no reference counterpart; src/lib.rs:33-52 per query): a
/// participant with several pending queries reads its resident share database once for all of
/// them.  `out[q]` receives what `DistanceEngine::new(&queries[q])` would write.
pub struct DistanceBatchEngine {
    h: Handle,
    nq: usize,
}

impl DistanceBatchEngine {
    pub fn new(queries: &[EncodedBits]) -> Self {
        Self::new_on(default_device(), queries).unwrap_or_else(|e| panic!("DistanceBatchEngine::new: {e}"))
    }

    /// 1..=IRIS_DISTANCE_BATCH_MAX queries.
    pub fn new_on(device: &Device, queries: &[EncodedBits]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::iris_distance_batch_engine_new(device.raw(), queries.as_ptr().cast(), queries.len() as u32, &mut raw)
        })?;
        Ok(Self { h: Handle { raw, _device: device.clone() }, nq: queries.len() })
    }

    pub fn nq(&self) -> usize {
        self.nq
    }

    /// Records [first, first + n) of a resident share database, n = `out[q].len()` for every q:
    /// out[q][i][k] = dot_u16(rot(queries[q], k - 15), db[first + i]).
    pub fn batch_process(&self, out: &mut [Vec<[u16; 31]>], db: &Database, first: u64) -> Result<()> {
        assert_eq!(out.len(), self.nq);
        let n = out.first().map_or(0, |o| o.len());
        assert!(out.iter().all(|o| o.len() == n), "output rows of different lengths");
        if n == 0 {
            return Ok(());
        }
        // the C call writes one query-major array
        let mut flat = vec![[0_u16; 31]; self.nq * n];
        check(unsafe {
            ffi::iris_distance_batch_process(self.h.raw, db.raw(), first, n as u64, flat.as_mut_ptr().cast())
        })?;
        for (q, o) in out.iter_mut().enumerate() {
            o.copy_from_slice(&flat[q * n..(q + 1) * n]);
        }
        Ok(())
    }

    /// The rows stay on the GPU: `out_device` is a DEVICE array of nq * n * 31 u16 (query-major).
    pub fn batch_process_device(&self, out_device: *mut u16, db: &Database, first: u64, n: u64) -> Result<()> {
        check(unsafe { ffi::iris_distance_batch_process_device(self.h.raw, db.raw(), first, n, out_device) })
    }
}

/// `MasksEngine` (src/lib.rs:55-80): out[i][k] = dot_bool(rot(query, k - 15), db[i]).
pub struct MasksEngine {
    h: Handle,
}

impl MasksEngine {
    pub fn new(query: &Bits) -> Self {
        Self::new_on(default_device(), query).unwrap_or_else(|e| panic!("MasksEngine::new: {e}"))
    }

    pub fn new_on(device: &Device, query: &Bits) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::iris_masks_engine_new(device.raw(), query.0.as_ptr(), &mut raw) })?;
        Ok(Self { h: Handle { raw, _device: device.clone() } })
    }

    pub fn batch_process(&self, out: &mut [[u16; 31]], db: &[Bits]) {
        self.h.batch_process_host("MasksEngine", out, db)
    }

    pub fn batch_process_resident(&self, out: &mut [[u16; 31]], db: &Database, first: u64) -> Result<()> {
        self.h.batch_process_resident(out, db, first)
    }

    /// The resolver's step in one pass (src/main.rs:510-519 + 597-621): denominators of
    /// masks [first, first + n) from this engine, the wrapping sum of the participants'
    /// share rows (DEVICE arrays of n x 31 u16), decode and first strict minimum.
    pub fn resolve(&self, masks: &Database, first: u64, n: u64, shares_device: &[*const u16]) -> Result<(f64, usize)> {
        let mut m = ffi::IrisMatch::default();
        check(unsafe {
            ffi::iris_resolver_search_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                0,
                ptr::null_mut(),
                &mut m,
            )
        })?;
        Ok(match_to_pair(&m))
    }

    /// Every record of that step whose decoded distance is below `threshold`
    /// (iris_resolver_matches_masks; the threshold has no reference counterpart): indices are the
    /// rows within the range.  -> (matches in ascending index order, total count).
    pub fn matches(
        &self,
        masks: &Database,
        first: u64,
        n: u64,
        shares_device: &[*const u16],
        threshold: f64,
        cap: Option<u64>,
    ) -> Result<(Vec<(f64, usize)>, u64)> {
        collect_matches(cap, |out, room, count| unsafe {
            ffi::iris_resolver_matches_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                0,
                threshold,
                out,
                room,
                count,
            )
        })
    }

    /// The k closest records of that step, best first (iris_resolver_topk_masks; k has no reference
    /// counterpart): indices are the rows within the range.
    pub fn topk(&self, masks: &Database, first: u64, n: u64, shares_device: &[*const u16], k: u32) -> Result<Vec<(f64, usize)>> {
        collect_topk(k, |out, count| unsafe {
            ffi::iris_resolver_topk_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                0,
                k,
                out,
                count,
            )
        })
    }

    /// The distance distribution of that step (iris_resolver_histogram_masks; no reference
    /// counterpart) -> (bins, invalid); `nbins` is a power of two up to `ffi::IRIS_HIST_MAX_BINS`.
    pub fn histogram(&self, masks: &Database, first: u64, n: u64, shares_device: &[*const u16], nbins: u32) -> Result<(Vec<u64>, u64)> {
        let mut bins = vec![0u64; nbins.clamp(1, ffi::IRIS_HIST_MAX_BINS) as usize];
        let mut invalid = 0u64;
        check(unsafe {
            ffi::iris_resolver_histogram_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                nbins,
                bins.as_mut_ptr(),
                &mut invalid,
            )
        })?;
        Ok((bins, invalid))
    }

    /// Several of `matches`, `topk` and `histogram` of that step from ONE masks pass
    /// (iris_resolver_report_masks; no reference counterpart).  Parts as in `TemplateEngine::report`;
    /// each selected part is exactly what the sibling method returns.
    pub fn report(
        &self,
        masks: &Database,
        first: u64,
        n: u64,
        shares_device: &[*const u16],
        index_base: u64,
        matches: Option<(f64, u64)>,
        k: Option<u32>,
        nbins: Option<u32>,
    ) -> Result<Report> {
        collect_report(matches, k, nbins, |r| unsafe {
            ffi::iris_resolver_report_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                index_base,
                r as *mut ffi::IrisReport as *mut _,
            )
        })
    }

    /// The same step with the participants' replies still in host memory (`shares[p]` holds the
    /// n = `shares[p].len()` rows of records [first, first + n)): the library sums the parts on
    /// the host and uploads only the sum (iris_resolver_search_masks_host).
    pub fn resolve_host(&self, masks: &Database, first: u64, shares: &[&[[u16; 31]]]) -> Result<(f64, usize)> {
        let n = shares.first().map_or(0, |s| s.len());
        assert!(shares.iter().all(|s| s.len() == n), "share arrays of different lengths");
        let ptrs: Vec<*const u16> = shares.iter().map(|s| s.as_ptr() as *const u16).collect();
        let mut m = ffi::IrisMatch::default();
        check(unsafe {
            ffi::iris_resolver_search_masks_host(
                self.h.raw,
                masks.raw(),
                first,
                n as u64,
                ptrs.as_ptr(),
                ptrs.len() as u32,
                0,
                &mut m,
            )
        })?;
        Ok(match_to_pair(&m))
    }
}

/// `nq` MasksEngines at once (no reference counterpart; the reference computes denominators and
/// decodes one query at a time, src/main.rs:506-519 and 597-621): a resolver with several pending
/// queries reads its resident masks database once for all of them.
pub struct MasksBatchEngine {
    h: Handle,
    nq: usize,
}

impl MasksBatchEngine {
    pub fn new(queries: &[Bits]) -> Self {
        Self::new_on(default_device(), queries).unwrap_or_else(|e| panic!("MasksBatchEngine::new: {e}"))
    }

    /// 1..=IRIS_MASKS_BATCH_MAX queries.
    pub fn new_on(device: &Device, queries: &[Bits]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::iris_masks_batch_engine_new(device.raw(), queries.as_ptr().cast(), queries.len() as u32, &mut raw)
        })?;
        Ok(Self { h: Handle { raw, _device: device.clone() }, nq: queries.len() })
    }

    pub fn nq(&self) -> usize {
        self.nq
    }

    /// Records [first, first + n) of a resident masks database, n = `out[q].len()` for every q:
    /// out[q][i][k] = dot_bool(rot(queries[q], k - 15), db[first + i]).
    pub fn batch_process(&self, out: &mut [Vec<[u16; 31]>], db: &Database, first: u64) -> Result<()> {
        assert_eq!(out.len(), self.nq);
        let n = out.first().map_or(0, |o| o.len());
        assert!(out.iter().all(|o| o.len() == n), "output rows of different lengths");
        if n == 0 {
            return Ok(());
        }
        // the C call writes one query-major array
        let mut flat = vec![[0_u16; 31]; self.nq * n];
        check(unsafe { ffi::iris_masks_batch_process(self.h.raw, db.raw(), first, n as u64, flat.as_mut_ptr().cast()) })?;
        for (q, o) in out.iter_mut().enumerate() {
            o.copy_from_slice(&flat[q * n..(q + 1) * n]);
        }
        Ok(())
    }

    /// The resolver's step for every query in one pass over masks [first, first + n):
    /// `shares_device[p]` is participant p's DEVICE array of nq x n x 31 u16, query-major (what
    /// `DistanceBatchEngine::batch_process_device` wrote over the same records).  One
    /// (distance, index) per query.
    pub fn resolve(&self, masks: &Database, first: u64, n: u64, shares_device: &[*const u16]) -> Result<Vec<(f64, usize)>> {
        let mut m = vec![ffi::IrisMatch::default(); self.nq];
        check(unsafe {
            ffi::iris_resolver_batch_search_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                0,
                ptr::null_mut(),
                m.as_mut_ptr(),
            )
        })?;
        Ok(m.iter().map(match_to_pair).collect())
    }

    /// Every query's records of that step whose decoded distance is below `threshold`, in one
    /// pass over the masks (iris_resolver_batch_matches_masks; the threshold has no reference
    /// counterpart): entry q is what `MasksEngine::matches` gives for query q on slab q of every
    /// part -- (matches in ascending index order, total count).  `cap` is per query; None asks
    /// for every match (room for 1024 a query first, then once more for the longest list).
    pub fn batch_matches(
        &self,
        masks: &Database,
        first: u64,
        n: u64,
        shares_device: &[*const u16],
        threshold: f64,
        cap: Option<u64>,
    ) -> Result<Vec<(Vec<(f64, usize)>, u64)>> {
        let mut room = cap.unwrap_or(1024);
        let mut counts = vec![0u64; self.nq];
        let mut pass = 0;
        let buf = loop {
            let mut buf = vec![ffi::IrisMatch::default(); self.nq * room as usize];
            check(unsafe {
                ffi::iris_resolver_batch_matches_masks(
                    self.h.raw,
                    masks.raw(),
                    first,
                    n,
                    shares_device.as_ptr(),
                    shares_device.len() as u32,
                    0,
                    threshold,
                    if room == 0 { ptr::null_mut() } else { buf.as_mut_ptr() },
                    room,
                    counts.as_mut_ptr(),
                )
            })?;
            let longest = counts.iter().copied().max().unwrap_or(0);
            if cap.is_some() || pass == 1 || longest <= room {
                break buf;
            }
            room = longest;
            pass += 1;
        };
        Ok(counts
            .iter()
            .enumerate()
            .map(|(q, &c)| {
                let list = &buf[q * room as usize..q * room as usize + c.min(room) as usize];
                (list.iter().map(match_to_pair).collect(), c)
            })
            .collect())
    }

    /// Every query's k closest records of that step, best first, in one pass over the masks
    /// (iris_resolver_batch_topk_masks; k = 1..=ffi::IRIS_TOPK_MAX has no reference counterpart):
    /// entry q is what `MasksEngine::topk` gives for query q on slab q of every part.
    pub fn batch_topk(
        &self,
        masks: &Database,
        first: u64,
        n: u64,
        shares_device: &[*const u16],
        k: u32,
    ) -> Result<Vec<Vec<(f64, usize)>>> {
        let room = k.clamp(1, ffi::IRIS_TOPK_MAX) as usize;
        let mut buf = vec![ffi::IrisMatch::default(); self.nq * room];
        let mut counts = vec![0u32; self.nq];
        check(unsafe {
            ffi::iris_resolver_batch_topk_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                0,
                k,
                buf.as_mut_ptr(),
                counts.as_mut_ptr(),
            )
        })?;
        Ok(counts
            .iter()
            .enumerate()
            .map(|(q, &c)| buf[q * room..q * room + c as usize].iter().map(match_to_pair).collect())
            .collect())
    }

    /// Every query's distance histogram of that step in one pass over the masks
    /// (iris_resolver_batch_histogram_masks): entry q is what `MasksEngine::histogram` gives for
    /// query q on slab q of every part.
    pub fn batch_histogram(
        &self,
        masks: &Database,
        first: u64,
        n: u64,
        shares_device: &[*const u16],
        nbins: u32,
    ) -> Result<Vec<(Vec<u64>, u64)>> {
        let room = nbins.clamp(1, ffi::IRIS_HIST_MAX_BINS) as usize;
        let mut flat = vec![0u64; self.nq * room];
        let mut invalid = vec![0u64; self.nq];
        check(unsafe {
            ffi::iris_resolver_batch_histogram_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                nbins,
                flat.as_mut_ptr(),
                invalid.as_mut_ptr(),
            )
        })?;
        Ok((0..self.nq).map(|q| (flat[q * room..(q + 1) * room].to_vec(), invalid[q])).collect())
    }

    /// Several of `batch_matches`, `batch_topk` and `batch_histogram` for every query from ONE pass
    /// over the masks and the share slabs (iris_resolver_batch_report_masks; no reference
    /// counterpart).  A part is selected by its argument: `matches = Some((threshold, cap))` with
    /// cap records a query (`0` only counts), `k`, `nbins`; one of each serves all queries.  Entry
    /// q holds the selected parts as those methods return them for query q; `topk[0]` at k = 1 is
    /// the batched resolve's entry q.
    pub fn batch_report(
        &self,
        masks: &Database,
        first: u64,
        n: u64,
        shares_device: &[*const u16],
        index_base: u64,
        matches: Option<(f64, u64)>,
        k: Option<u32>,
        nbins: Option<u32>,
    ) -> Result<Vec<Report>> {
        batch_report_call(self.nq, matches, k, nbins, |r| unsafe {
            ffi::iris_resolver_batch_report_masks(
                self.h.raw,
                masks.raw(),
                first,
                n,
                shares_device.as_ptr(),
                shares_device.len() as u32,
                index_base,
                r,
            )
        })
    }
}

/// One batch report call (iris_template_batch_report, iris_resolver_batch_report_masks) for nq
/// queries: `call(report)` with the IrisBatchReport filled from the selected parts' arguments, then
/// entry q's selected parts from its arrays.
fn batch_report_call(
    nq: usize,
    matches: Option<(f64, u64)>,
    k: Option<u32>,
    nbins: Option<u32>,
    call: impl FnOnce(*mut std::ffi::c_void) -> std::os::raw::c_int,
) -> Result<Vec<Report>> {
    let mut r = ffi::IrisBatchReport {
        parts: 0,
        k: 0,
        nbins: 0,
        reserved: 0,
        threshold: 0.0,
        matches: ptr::null_mut(),
        matches_cap: 0,
        matches_counts: ptr::null_mut(),
        topk: ptr::null_mut(),
        topk_counts: ptr::null_mut(),
        bins: ptr::null_mut(),
        invalid: ptr::null_mut(),
    };
    let cap = matches.map_or(0, |m| m.1);
    let kroom = k.unwrap_or(1).clamp(1, ffi::IRIS_TOPK_MAX) as usize;
    let broom = nbins.unwrap_or(1).clamp(1, ffi::IRIS_HIST_MAX_BINS) as usize;
    let mut lists = vec![ffi::IrisMatch::default(); nq * cap as usize];
    let mut totals = vec![0u64; nq];
    let mut best = vec![ffi::IrisMatch::default(); if k.is_some() { nq * kroom } else { 0 }];
    let mut listed = vec![0u32; nq];
    let mut bins = vec![0u64; if nbins.is_some() { nq * broom } else { 0 }];
    let mut invalid = vec![0u64; nq];
    if let Some((threshold, _)) = matches {
        r.parts |= ffi::IRIS_REPORT_MATCHES;
        r.threshold = threshold;
        r.matches_cap = cap;
        r.matches = if cap == 0 { ptr::null_mut() } else { lists.as_mut_ptr() };
        r.matches_counts = totals.as_mut_ptr();
    }
    if let Some(k) = k {
        r.parts |= ffi::IRIS_REPORT_TOPK;
        r.k = k;
        r.topk = best.as_mut_ptr();
        r.topk_counts = listed.as_mut_ptr();
    }
    if let Some(nbins) = nbins {
        r.parts |= ffi::IRIS_REPORT_HIST;
        r.nbins = nbins;
        r.bins = bins.as_mut_ptr();
        r.invalid = invalid.as_mut_ptr();
    }
    check(call(&mut r as *mut ffi::IrisBatchReport as *mut _))?;
    Ok((0..nq)
        .map(|q| Report {
            matches: matches.map(|_| {
                let list = &lists[q * cap as usize..q * cap as usize + totals[q].min(cap) as usize];
                (list.iter().map(match_to_pair).collect(), totals[q])
            }),
            topk: k.map(|_| best[q * kroom..q * kroom + listed[q] as usize].iter().map(match_to_pair).collect()),
            histogram: nbins.map(|_| (bins[q * broom..(q + 1) * broom].to_vec(), invalid[q])),
        })
        .collect())
}

/// `distances` (src/lib.rs:82-87).
pub fn distances(query: &EncodedBits, entry: &EncodedBits) -> [u16; 31] {
    let mut result = [0_u16; 31];
    DistanceEngine::new(query).batch_process(std::slice::from_mut(&mut result), std::slice::from_ref(entry));
    result
}

/// `denominators` (src/lib.rs:89-94).
pub fn denominators(query: &Bits, entry: &Bits) -> [u16; 31] {
    let mut result = [0_u16; 31];
    MasksEngine::new(query).batch_process(std::slice::from_mut(&mut result), std::slice::from_ref(entry));
    result
}

/// Plaintext masked Hamming of one query against a resident Template database:
/// `Template::distance` per record (src/template.rs:43-64) and the resolver's
/// `(min_distance, min_index)` (src/main.rs:616-621), bit-exact.
pub struct TemplateEngine {
    h: Handle,
    query: Template,
}

/// An enqueued search (`iris_template_search_async`); `wait` blocks for it alone.
pub struct PendingSearch {
    raw: *mut ffi::IrisPending,
}

unsafe impl Send for PendingSearch {}

impl PendingSearch {
    pub fn wait(mut self) -> Result<(f64, usize)> {
        let mut m = ffi::IrisMatch::default();
        let raw = std::mem::replace(&mut self.raw, ptr::null_mut());
        check(unsafe { ffi::iris_pending_wait(raw, &mut m) })?;
        Ok(match_to_pair(&m))
    }
}

impl Drop for PendingSearch {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            let mut m = ffi::IrisMatch::default();
            unsafe {
                ffi::iris_pending_wait(self.raw, &mut m);
            }
        }
    }
}

/// An enqueued threshold-match pass (`iris_template_matches_async`); `wait` blocks for it alone
/// and returns what `TemplateEngine::matches` with `Some(cap)` returns.
pub struct PendingMatches {
    raw: *mut ffi::IrisPendingMatches,
    cap: u64,
}

unsafe impl Send for PendingMatches {}

impl PendingMatches {
    pub fn wait(mut self) -> Result<(Vec<(f64, usize)>, u64)> {
        let raw = std::mem::replace(&mut self.raw, ptr::null_mut());
        collect_matches(Some(self.cap), |out, _room, count| unsafe { ffi::iris_pending_matches_wait(raw, out, count) })
    }
}

impl Drop for PendingMatches {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            let mut count = 0u64;
            unsafe {
                ffi::iris_pending_matches_wait(self.raw, ptr::null_mut(), &mut count);
            }
        }
    }
}

/// An enqueued top-k pass (`iris_template_topk_async`); `wait` blocks for it alone and returns
/// what `TemplateEngine::topk` returns.
pub struct PendingTopk {
    raw: *mut ffi::IrisPendingTopk,
    k: u32,
}

unsafe impl Send for PendingTopk {}

impl PendingTopk {
    pub fn wait(mut self) -> Result<Vec<(f64, usize)>> {
        let raw = std::mem::replace(&mut self.raw, ptr::null_mut());
        collect_topk(self.k, |out, count| unsafe { ffi::iris_pending_topk_wait(raw, out, count) })
    }
}

impl Drop for PendingTopk {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            let mut count = 0u32;
            unsafe {
                ffi::iris_pending_topk_wait(self.raw, ptr::null_mut(), &mut count);
            }
        }
    }
}

/// An enqueued report pass (`iris_template_report_async`); `wait` blocks for it alone and returns
/// what `TemplateEngine::report` returns for the same parts.
pub struct PendingReport {
    raw: *mut ffi::IrisPendingReport,
    matches: Option<(f64, u64)>,
    k: Option<u32>,
    nbins: Option<u32>,
}

unsafe impl Send for PendingReport {}

impl PendingReport {
    pub fn wait(mut self) -> Result<Report> {
        let raw = std::mem::replace(&mut self.raw, ptr::null_mut());
        collect_report(self.matches, self.k, self.nbins, |r| unsafe {
            ffi::iris_pending_report_wait(raw, r as *mut ffi::IrisReport as *mut _)
        })
    }
}

impl Drop for PendingReport {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            unsafe {
                ffi::iris_pending_report_wait(self.raw, ptr::null_mut()); // refused, and the handle freed
            }
        }
    }
}

impl TemplateEngine {
    pub fn new(query: &Template) -> Self {
        Self::new_on(default_device(), query).unwrap_or_else(|e| panic!("TemplateEngine::new: {e}"))
    }

    pub fn new_on(device: &Device, query: &Template) -> Result<Self> {
        let mut raw = ptr::null_mut();
        let q = query as *const Template as *const ffi::IrisTemplate;
        check(unsafe { ffi::iris_template_engine_new(device.raw(), q, &mut raw) })?;
        Ok(Self { h: Handle { raw, _device: device.clone() }, query: *query })
    }

    /// The same query over a sharded multi-GPU database (every device builds its own
    /// engine, searches its shards; winners all-gathered over RCCL and merged).
    pub fn search_sharded(&self, db: &ShardedDatabase) -> Result<(f64, usize)> {
        db.search(&self.query)
    }

    /// `Template::distance(query, db[i])` for i in [first, first + out.len()).
    pub fn distances(&self, db: &Database, first: u64, out: &mut [f64]) -> Result<()> {
        check(unsafe { ffi::iris_template_distances(self.h.raw, db.raw(), first, out.len() as u64, out.as_mut_ptr()) })
    }

    /// Min / argmin over records [first, first + n); indices are `index_base + i`.
    pub fn search(&self, db: &Database, first: u64, n: u64, index_base: u64) -> Result<(f64, usize)> {
        let mut m = ffi::IrisMatch::default();
        check(unsafe {
            ffi::iris_template_search(self.h.raw, db.raw(), first, n, index_base, ptr::null_mut(), &mut m)
        })?;
        Ok(match_to_pair(&m))
    }

    /// Every record of [first, first + n) whose distance is below `threshold`, in one database
    /// pass (iris_template_matches; the threshold has no reference counterpart); indices are
    /// `index_base + first + i`.  -> (matches in ascending index order, total count).
    pub fn matches(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        threshold: f64,
        cap: Option<u64>,
    ) -> Result<(Vec<(f64, usize)>, u64)> {
        collect_matches(cap, |out, room, count| unsafe {
            ffi::iris_template_matches(self.h.raw, db.raw(), first, n, index_base, threshold, out, room, count)
        })
    }

    /// Enqueues `matches` with `Some(cap)` and returns at once (iris_template_matches_async): a pass
    /// still running may compute the next one submitted.  The engine may be dropped before the
    /// wait; the database must outlive it, unmodified.
    pub fn matches_async(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        threshold: f64,
        cap: u64,
    ) -> Result<PendingMatches> {
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::iris_template_matches_async(self.h.raw, db.raw(), first, n, index_base, threshold, cap, &mut raw)
        })?;
        Ok(PendingMatches { raw, cap })
    }

    /// The k closest records of [first, first + n), best first, in one database pass
    /// (iris_template_topk; k has no reference counterpart); indices are `index_base + first + i`.
    pub fn topk(&self, db: &Database, first: u64, n: u64, index_base: u64, k: u32) -> Result<Vec<(f64, usize)>> {
        collect_topk(k, |out, count| unsafe {
            ffi::iris_template_topk(self.h.raw, db.raw(), first, n, index_base, k, out, count)
        })
    }

    /// The distribution of the distances of [first, first + n) in one database pass
    /// (iris_template_histogram; no reference counterpart) -> (bins, invalid): a record is counted
    /// in bin `min(nbins - 1, floor(distance * nbins))`, one without a valid rotation in `invalid`
    /// alone.  `nbins` is a power of two up to `ffi::IRIS_HIST_MAX_BINS`; histograms of chunks add.
    pub fn histogram(&self, db: &Database, first: u64, n: u64, nbins: u32) -> Result<(Vec<u64>, u64)> {
        let mut bins = vec![0u64; nbins.clamp(1, ffi::IRIS_HIST_MAX_BINS) as usize];
        let mut invalid = 0u64;
        check(unsafe {
            ffi::iris_template_histogram(self.h.raw, db.raw(), first, n, nbins, bins.as_mut_ptr(), &mut invalid)
        })?;
        Ok((bins, invalid))
    }

    /// Several of `matches`, `topk` and `histogram` from ONE read of [first, first + n)
    /// (iris_template_report; no reference counterpart).  A part is selected by its argument:
    /// `matches = Some((threshold, cap))` (the `cap` lowest indices and the exact total; 0 only
    /// counts), `k = Some(k)`, `nbins = Some(nbins)`; at least one.  Each selected part of the result
    /// is exactly what the sibling method returns, the others are `None`.
    pub fn report(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        matches: Option<(f64, u64)>,
        k: Option<u32>,
        nbins: Option<u32>,
    ) -> Result<Report> {
        collect_report(matches, k, nbins, |r| unsafe {
            ffi::iris_template_report(self.h.raw, db.raw(), first, n, index_base, r as *mut ffi::IrisReport as *mut _)
        })
    }

    /// Enqueues `report` and returns at once (iris_template_report_async): a report pass still
    /// running may compute the next one submitted, whatever parts and arguments the two ask for;
    /// `nbins` alone is the pipelined histogram.  The engine may be dropped before the wait; the
    /// database must outlive it, unmodified.
    pub fn report_async(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        matches: Option<(f64, u64)>,
        k: Option<u32>,
        nbins: Option<u32>,
    ) -> Result<PendingReport> {
        // the in scalars only: the submission reads no pointer
        let mut r = ffi::IrisReport {
            parts: 0,
            k: k.unwrap_or(0),
            nbins: nbins.unwrap_or(0),
            topk_count: 0,
            threshold: matches.map_or(0.0, |m| m.0),
            matches: ptr::null_mut(),
            matches_cap: matches.map_or(0, |m| m.1),
            matches_count: 0,
            topk: ptr::null_mut(),
            bins: ptr::null_mut(),
            invalid: 0,
        };
        if matches.is_some() {
            r.parts |= ffi::IRIS_REPORT_MATCHES;
        }
        if k.is_some() {
            r.parts |= ffi::IRIS_REPORT_TOPK;
        }
        if nbins.is_some() {
            r.parts |= ffi::IRIS_REPORT_HIST;
        }
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::iris_template_report_async(
                self.h.raw,
                db.raw(),
                first,
                n,
                index_base,
                &r as *const ffi::IrisReport as *const _,
                &mut raw,
            )
        })?;
        Ok(PendingReport { raw, matches, k, nbins })
    }

    /// Enqueues `topk` and returns at once (iris_template_topk_async): a pass still running may
    /// compute the next one submitted.  The engine may be dropped before the wait; the database
    /// must outlive it, unmodified.
    pub fn topk_async(&self, db: &Database, first: u64, n: u64, index_base: u64, k: u32) -> Result<PendingTopk> {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::iris_template_topk_async(self.h.raw, db.raw(), first, n, index_base, k, &mut raw) })?;
        Ok(PendingTopk { raw, k })
    }

    /// Enqueues the search and returns at once (the engine may be dropped before the
    /// wait; the database must outlive it).
    pub fn search_async(&self, db: &Database, first: u64, n: u64, index_base: u64) -> Result<PendingSearch> {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::iris_template_search_async(self.h.raw, db.raw(), first, n, index_base, &mut raw) })?;
        Ok(PendingSearch { raw })
    }
}

/// Many query Templates against one resident Template database in one pass (no reference
/// counterpart; the reference folds one query at a time, src/template.rs:43-47 and
/// src/main.rs:616-621): a deduplication run or a plaintext identification service with many
/// probes reads the enrolled database once for all of them.
pub struct TemplateBatchEngine {
    h: Handle,
    nq: usize,
}

impl TemplateBatchEngine {
    pub fn new(queries: &[Template]) -> Self {
        Self::new_on(default_device(), queries).unwrap_or_else(|e| panic!("TemplateBatchEngine::new: {e}"))
    }

    /// At least one query; more than 3 need a database in the TILES layout.
    pub fn new_on(device: &Device, queries: &[Template]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::iris_template_batch_engine_new(device.raw(), queries.as_ptr().cast(), queries.len() as u32, &mut raw)
        })?;
        Ok(Self { h: Handle { raw, _device: device.clone() }, nq: queries.len() })
    }

    pub fn nq(&self) -> usize {
        self.nq
    }

    /// Every query's (min distance, index) over records [first, first + n); indices are
    /// `index_base + first + i`.
    pub fn batch_search(&self, db: &Database, first: u64, n: u64, index_base: u64) -> Result<Vec<(f64, usize)>> {
        let mut m = vec![ffi::IrisMatch::default(); self.nq];
        check(unsafe { ffi::iris_template_batch_search(self.h.raw, db.raw(), first, n, index_base, m.as_mut_ptr()) })?;
        Ok(m.iter().map(match_to_pair).collect())
    }

    /// Every query's records of [first, first + n) whose distance is below `threshold`, in one
    /// pass over the templates (iris_template_batch_matches; the threshold has no reference
    /// counterpart): entry q is what `TemplateEngine::matches` gives for query q -- (matches in
    /// ascending index order, total count).  `cap` is per query; None asks for every match (room
    /// for at most 1024 a query first, 64 at 1024 queries, then once more for the longest list).
    pub fn batch_matches(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        threshold: f64,
        cap: Option<u64>,
    ) -> Result<Vec<(Vec<(f64, usize)>, u64)>> {
        let mut room = cap.unwrap_or((65536 / self.nq.max(1) as u64).clamp(16, 1024));
        let mut counts = vec![0u64; self.nq];
        let mut pass = 0;
        let buf = loop {
            let mut buf = vec![ffi::IrisMatch::default(); self.nq * room as usize];
            check(unsafe {
                ffi::iris_template_batch_matches(
                    self.h.raw,
                    db.raw(),
                    first,
                    n,
                    index_base,
                    threshold,
                    if room == 0 { ptr::null_mut() } else { buf.as_mut_ptr() },
                    room,
                    counts.as_mut_ptr(),
                )
            })?;
            let longest = counts.iter().copied().max().unwrap_or(0);
            if cap.is_some() || pass == 1 || longest <= room {
                break buf;
            }
            room = longest;
            pass += 1;
        };
        Ok(counts
            .iter()
            .enumerate()
            .map(|(q, &c)| {
                let list = &buf[q * room as usize..q * room as usize + c.min(room) as usize];
                (list.iter().map(match_to_pair).collect(), c)
            })
            .collect())
    }

    /// Every query's k closest records of [first, first + n), best first, in one pass over the
    /// templates (iris_template_batch_topk; k = 1..=ffi::IRIS_TOPK_MAX has no reference
    /// counterpart): entry q is what `TemplateEngine::topk` gives for query q; indices are
    /// `index_base + first + i`.
    pub fn batch_topk(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        k: u32,
    ) -> Result<Vec<Vec<(f64, usize)>>> {
        let room = k.clamp(1, ffi::IRIS_TOPK_MAX) as usize;
        let mut buf = vec![ffi::IrisMatch::default(); self.nq * room];
        let mut counts = vec![0u32; self.nq];
        check(unsafe {
            ffi::iris_template_batch_topk(
                self.h.raw,
                db.raw(),
                first,
                n,
                index_base,
                k,
                buf.as_mut_ptr(),
                counts.as_mut_ptr(),
            )
        })?;
        Ok(counts
            .iter()
            .enumerate()
            .map(|(q, &c)| buf[q * room..q * room + c as usize].iter().map(match_to_pair).collect())
            .collect())
    }

    /// Every query's distance histogram of [first, first + n) in one pass over the templates
    /// (iris_template_batch_histogram): entry q is what `TemplateEngine::histogram` gives for
    /// query q.
    pub fn batch_histogram(&self, db: &Database, first: u64, n: u64, nbins: u32) -> Result<Vec<(Vec<u64>, u64)>> {
        let room = nbins.clamp(1, ffi::IRIS_HIST_MAX_BINS) as usize;
        let mut bins = vec![0u64; self.nq * room];
        let mut invalid = vec![0u64; self.nq];
        check(unsafe {
            ffi::iris_template_batch_histogram(
                self.h.raw,
                db.raw(),
                first,
                n,
                nbins,
                bins.as_mut_ptr(),
                invalid.as_mut_ptr(),
            )
        })?;
        Ok(invalid
            .iter()
            .enumerate()
            .map(|(q, &inv)| (bins[q * room..(q + 1) * room].to_vec(), inv))
            .collect())
    }

    /// Several of `batch_matches`, `batch_topk` and `batch_histogram` for every query from ONE pass
    /// over the templates (iris_template_batch_report; no reference counterpart).  A part is
    /// selected by its argument: `matches = Some((threshold, cap))` with cap records a query
    /// (`0` only counts), `k`, `nbins`; one of each serves all queries.  Entry q holds the
    /// selected parts as those methods return them for query q.
    pub fn batch_report(
        &self,
        db: &Database,
        first: u64,
        n: u64,
        index_base: u64,
        matches: Option<(f64, u64)>,
        k: Option<u32>,
        nbins: Option<u32>,
    ) -> Result<Vec<Report>> {
        batch_report_call(self.nq, matches, k, nbins, |r| unsafe {
            ffi::iris_template_batch_report(self.h.raw, db.raw(), first, n, index_base, r)
        })
    }
}

#[cfg(test)]
mod tests {
    //! The reference's engine semantics against plain host loops (wrapping u16 MACs and
    //! popcounts over the reference's own rotations), on random records.
    use super::*;
    use rand::{thread_rng, Rng};

    #[test]
    fn distance_engine_matches_host_loop() {
        let mut rng = thread_rng();
        let q: EncodedBits = rng.gen();
        let db: Vec<EncodedBits> = (0..37).map(|_| rng.gen()).collect();
        let mut out = vec![[0u16; 31]; db.len()];
        DistanceEngine::new(&q).batch_process(&mut out, &db);
        for (row, e) in out.iter().zip(db.iter()) {
            for (k, &got) in row.iter().enumerate() {
                let r = q.rotated(k as i32 - 15);
                let want = r.0.iter().zip(e.0.iter()).fold(0u16, |s, (&a, &b)| s.wrapping_add(a.wrapping_mul(b)));
                assert_eq!(got, want);
            }
        }
    }

    #[test]
    fn masks_engine_matches_host_loop() {
        let mut rng = thread_rng();
        let q: Bits = rng.gen();
        let db: Vec<Bits> = (0..37).map(|_| rng.gen()).collect();
        let mut out = vec![[0u16; 31]; db.len()];
        MasksEngine::new(&q).batch_process(&mut out, &db);
        for (row, e) in out.iter().zip(db.iter()) {
            for (k, &got) in row.iter().enumerate() {
                let r = q.rotated(k as i32 - 15);
                let want: u32 = r.0.iter().zip(e.0.iter()).map(|(&a, &b)| (a & b).count_ones()).sum();
                assert_eq!(got as u32, want);
            }
        }
    }

    #[test]
    #[should_panic]
    fn batch_process_length_mismatch_panics() {
        let mut rng = thread_rng();
        let q: Bits = rng.gen();
        let db: Vec<Bits> = (0..3).map(|_| rng.gen()).collect();
        let mut out = vec![[0u16; 31]; 2];
        MasksEngine::new(&q).batch_process(&mut out, &db);
    }

    #[test]
    fn template_search_matches_template_distance() {
        let mut rng = thread_rng();
        let query: Template = rng.gen();
        let mut records: Vec<Template> = (0..100).map(|_| rng.gen()).collect();
        records[61] = query.rotated(7);
        let dev = default_device();
        let mut db = Database::new::<Template>(dev, records.len() as u64).unwrap();
        db.append(&records).unwrap();
        let engine = TemplateEngine::new(&query);
        let mut d = vec![0f64; records.len()];
        engine.distances(&db, 0, &mut d).unwrap();
        for (got, r) in d.iter().zip(records.iter()) {
            assert_eq!(got.to_bits(), query.distance(r).to_bits());
        }
        let (best, index) = engine.search(&db, 0, records.len() as u64, 0).unwrap();
        assert_eq!((best, index), (0.0, 61));
    }

    #[test]
    fn attached_slices_match_host_loop() {
        // the resolver's loop (src/main.rs:511-516) over an attached array: no upload per chunk
        let mut rng = thread_rng();
        let q: Bits = rng.gen();
        let masks: Vec<Bits> = (0..5000).map(|_| rng.gen()).collect();
        let att = crate::iris_hip::AttachedDatabase::new(default_device(), &masks).unwrap();
        let engine = MasksEngine::new(&q);
        for chunk in masks.chunks(1234) {
            let mut out = vec![[0u16; 31]; chunk.len()];
            engine.batch_process(&mut out, chunk);
            for (row, e) in out.iter().zip(chunk.iter()) {
                for (k, &got) in row.iter().enumerate() {
                    let r = q.rotated(k as i32 - 15);
                    let want: u32 = r.0.iter().zip(e.0.iter()).map(|(&a, &b)| (a & b).count_ones()).sum();
                    assert_eq!(got as u32, want);
                }
            }
        }
        drop(att);
    }

    #[test]
    fn sharded_search_matches_single_device() {
        let mut rng = thread_rng();
        let query: Template = rng.gen();
        let mut records: Vec<Template> = (0..1000).map(|_| rng.gen()).collect();
        records[777] = query.rotated(-4);
        let group = crate::iris_hip::Group::new(&[0]).unwrap();
        let mut sdb = ShardedDatabase::new(&group, records.len() as u64, ffi::IRIS_LAYOUT_DEFAULT, 4).unwrap();
        sdb.write(0, &records).unwrap();
        let engine = TemplateEngine::new(&query);
        assert_eq!(engine.search_sharded(&sdb).unwrap(), (0.0, 777));
    }
}
