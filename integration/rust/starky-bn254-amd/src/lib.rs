//! Rust face of libsbn254.so for qope/starky-bn254: starky 0.1.1's `prove` and `verify_stark_proof` WITH THEIR OWN
//! SIGNATURES over the C ABI of include/sbn.h, so that the reference's call sites -- the tests
//! (src/curves/g1/exp.rs:818-826) and `*StarkyProofGenerator::run_once` (src/curves/g1/circuit.rs:192-200 and its G2 /
//! Fq12 siblings) -- switch to the MI355X path by changing `use starky::prover::prove` / `use
//! starky::verifier::verify_stark_proof` to `use starky_bn254_amd::{prove, verify_stark_proof}` and adding one
//! `impl SbnTable` per table; the call expressions themselves stay as they are:
//!
//! ```ignore
//! let inner_proof = prove::<F, C, _, D>(stark, &inner_config, trace, pi.try_into().unwrap(), &mut TimingTree::default()).unwrap();
//! verify_stark_proof(stark, inner_proof.clone(), &inner_config).unwrap();
//! ```
//!
//! SOURCE ONLY -- written without a Rust toolchain in the build image and never compiled there.  What is tested is
//! the C ABI below it (tests/test_gpu_parity.py through ctypes) and, textually, that these signatures have the argument
//! lists of the reference's call sites (tests/test_product_host.py); the struct field names follow starky/plonky2 at
//! rev 541e127 as recalled, so expect to touch `convert.rs` if that fork renamed a field.
pub mod convert;
pub mod ffi;

use anyhow::{anyhow, ensure, Result};
use plonky2::field::extension::Extendable;
use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::hash::hash_types::RichField;
use plonky2::hash::poseidon::PoseidonHash;
use plonky2::plonk::config::GenericConfig;
use plonky2::util::timing::TimingTree;
use starky::config::StarkConfig;
use starky::proof::StarkProofWithPublicInputs;
use starky::stark::Stark;
use std::ffi::CStr;
use std::ptr;

/// A table of the reference named the way the C ABI names it: (kind, num_io).  Implemented in the reference crate for
/// its stark types, e.g. `impl SbnTable for G1ExpStark<F, D> { fn desc(&self) -> (i32, usize) { (ffi::SBN_AIR_G1_EXP, self.num_io) } }`
/// (G1ExpStark keeps `num_io`, src/curves/g1/exp.rs:232-236).
pub trait SbnTable {
    fn desc(&self) -> (i32, usize);
}

fn air(t: &impl SbnTable) -> ffi::sbn_air_desc {
    let (kind, num_io) = t.desc();
    ffi::sbn_air_desc { kind, num_io: num_io as u32 }
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(ffi::sbn_last_error()).to_string_lossy().into_owned() }
}

fn check(rc: i32, what: &str) -> Result<()> {
    if rc == 0 {
        Ok(())
    } else {
        Err(anyhow!("{what} failed ({rc}): {}", last_error()))
    }
}

/// Which FRI the linked plonky2 speaks (include/sbn.h `sbn_config.fri_variant`): 1 = SBN_FRI_TIMES_X, 2 = SBN_FRI_PLAIN.
pub const FRI_VARIANT: u32 = 1;

/// `StarkConfig` -> `sbn_config`.  Only `FriReductionStrategy::ConstantArityBits` is supported, which is what
/// `standard_fast_config` uses (exp.rs:250-253).
pub fn to_sbn_config(c: &StarkConfig) -> Result<ffi::sbn_config> {
    use plonky2::fri::reduction_strategies::FriReductionStrategy::ConstantArityBits;
    let (arity_bits, final_poly_bits) = match c.fri_config.reduction_strategy {
        ConstantArityBits(a, f) => (a as u32, f as u32),
        _ => return Err(anyhow!("only ConstantArityBits FRI reduction is supported")),
    };
    Ok(ffi::sbn_config {
        security_bits: c.security_bits as u32,
        num_challenges: c.num_challenges as u32,
        rate_bits: c.fri_config.rate_bits as u32,
        cap_height: c.fri_config.cap_height as u32,
        proof_of_work_bits: c.fri_config.proof_of_work_bits,
        fri_arity_bits: arity_bits,
        fri_final_poly_bits: final_poly_bits,
        num_query_rounds: c.fri_config.num_query_rounds as u32,
        // plonky2 0.1.3 @ 541e127 (the fork this crate links) still multiplies the final polynomial by X in
        // fri/oracle.rs::prove_openings; set to 2 (SBN_FRI_PLAIN) when building against a plonky2 that dropped the step.
        fri_variant: FRI_VARIANT,
    })
}

/// include/sbn.h `sbn_config_for_rate`: `standard_fast_config` at another blowup and the same conjectured security (84 / 42 / 28
/// queries at `rate_bits` 1 / 2 / 3; 3 = the FRI parameters of plonky2's `standard_recursion_config`).  The provers and verifiers
/// accept `rate_bits` 1 and 3.  `to_sbn_config` passes a `StarkConfig`'s own `fri_config.rate_bits` through unchanged.
pub fn sbn_config_for_rate(rate_bits: u32) -> ffi::sbn_config {
    let mut c = ffi::sbn_config::default();
    unsafe { ffi::sbn_config_for_rate(rate_bits, &mut c) };
    c.fri_variant = FRI_VARIANT;
    c
}

/// Device context for one (table, degree_bits): HBM buffers, streams, twiddles.  Create once, prove many times.
pub struct Prover {
    raw: *mut ffi::sbn_prover,
    num_io: usize,
    n_pi: usize,
    n_cols: usize,
    degree_bits: usize,
    io_words: usize,
    blocks: Vec<ConstraintBlock>,
    num_zs: usize,
}
// one prover belongs to one thread at a time (include/sbn.h, "Threading")
unsafe impl Send for Prover {}

/// How a prover context stores the LDEs of its wide matrices (include/sbn.h, sbn_prover_options.lde_storage).
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)]
pub enum LdeStorage {
    /// every LDE whole in device memory
    #[default]
    Full,
    /// rate_bits > 1: only the rows the quotient reads are kept, the opened rows are recomputed from the coefficients; same proofs
    Compact,
}

/// Which verifier a prover runs on every proof before it returns it (include/sbn.h, sbn_prover_set_guard).
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)]
pub enum Guard {
    /// no check: the proof is returned as assembled
    #[default]
    Off,
    /// a device verifier of batch 1 that the prover owns, created by its first guarded proof
    Device,
    /// the host verifier (sbn_verify) on the calling thread
    Host,
}

impl Guard {
    fn raw(self) -> u32 {
        match self {
            Guard::Off => ffi::SBN_GUARD_OFF,
            Guard::Device => ffi::SBN_GUARD_DEVICE,
            Guard::Host => ffi::SBN_GUARD_HOST,
        }
    }
}

#[derive(Clone, Copy, Debug, Default)]
pub struct ProverOptions {
    pub lde_storage: LdeStorage,
}

impl ProverOptions {
    fn raw(&self) -> ffi::sbn_prover_options {
        ffi::sbn_prover_options {
            struct_size: std::mem::size_of::<ffi::sbn_prover_options>() as u32,
            lde_storage: if self.lde_storage == LdeStorage::Compact { ffi::SBN_LDE_COMPACT } else { ffi::SBN_LDE_FULL },
        }
    }
}

/// Device bytes `Prover::with_options` allocates at creation (sbn_prover_memory_plan); needs no device.
pub fn prover_memory_plan(stark: &impl SbnTable, config: &StarkConfig, degree_bits: usize, options: &ProverOptions) -> Result<u64> {
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let opt = options.raw();
    let mut bytes = 0u64;
    check(unsafe { ffi::sbn_prover_memory_plan(&a, &cfg, degree_bits as u32, &opt, &mut bytes) }, "sbn_prover_memory_plan")?;
    Ok(bytes)
}

impl Prover {
    pub fn new(stark: &impl SbnTable, config: &StarkConfig, degree_bits: usize) -> Result<Self> {
        Self::with_options(stark, config, degree_bits, &ProverOptions::default())
    }

    pub fn with_options(stark: &impl SbnTable, config: &StarkConfig, degree_bits: usize, options: &ProverOptions) -> Result<Self> {
        let a = air(stark);
        let cfg = to_sbn_config(config)?;
        let opt = options.raw();
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::sbn_prover_create_with(&a, &cfg, degree_bits as u32, &opt, &mut raw) }, "sbn_prover_create_with")?;
        // u32 words of one instance in `ios` (include/sbn.h, per table)
        let io_words = match a.kind {
            ffi::SBN_AIR_G1_EXP => 40,
            ffi::SBN_AIR_G2_EXP => 72,
            ffi::SBN_AIR_FQ12_EXP => 200,
            ffi::SBN_AIR_FQ_EXP => 24,
            ffi::SBN_AIR_FQ12_EXP_U64 => 194,
            _ => 0,
        };
        Ok(Self {
            raw,
            num_io: a.num_io as usize,
            n_pi: unsafe { ffi::sbn_air_num_public_inputs(&a) },
            n_cols: unsafe { ffi::sbn_air_num_columns(&a) },
            degree_bits,
            io_words,
            blocks: constraint_blocks_of(&a),
            num_zs: unsafe { ffi::sbn_air_num_permutation_zs(&a, &cfg) },
        })
    }

    /// The blocks of the table's constraint stream (sbn_air_constraint_blocks): what `explain_rows` / `explain_trace` name.
    pub fn constraint_blocks(&self) -> &[ConstraintBlock] {
        &self.blocks
    }

    /// Which constraint blocks and permutation Z columns the listed rows of the loaded trace break (sbn_prover_explain_rows).
    /// A block is the granularity: inside a merged block the factored sums cannot separate constraints (include/sbn.h).
    pub fn explain_rows(&mut self, rows: &[u64], seed: u64) -> Result<Vec<RowExplanation>> {
        let (bb, zb) = ((self.blocks.len() + 7) / 8, (self.num_zs + 7) / 8);
        let (mut bf, mut zf) = (vec![0u8; rows.len() * bb], vec![0u8; rows.len() * zb]);
        check(
            unsafe { ffi::sbn_prover_explain_rows(self.raw, seed, rows.as_ptr(), rows.len(), bf.as_mut_ptr(), zf.as_mut_ptr()) },
            "sbn_prover_explain_rows",
        )?;
        let set = |bits: &[u8], n: usize| (0..n).filter(|i| (bits[i >> 3] >> (i & 7)) & 1 == 1).collect::<Vec<usize>>();
        Ok(rows
            .iter()
            .enumerate()
            .map(|(k, &r)| RowExplanation { row: r as usize, blocks: set(&bf[k * bb..(k + 1) * bb], self.blocks.len()), zs: set(&zf[k * zb..(k + 1) * zb], self.num_zs) })
            .collect())
    }

    /// Per block and per Z column, on how many rows of the loaded trace it fails and where first (sbn_prover_explain_trace).
    pub fn explain_trace(&mut self, seed: u64) -> Result<TraceExplanation> {
        let mut bs = vec![ffi::sbn_block_stat::default(); self.blocks.len()];
        let mut zs = vec![ffi::sbn_block_stat::default(); self.num_zs];
        check(unsafe { ffi::sbn_prover_explain_trace(self.raw, seed, bs.as_mut_ptr(), zs.as_mut_ptr()) }, "sbn_prover_explain_trace")?;
        let stat = |s: &ffi::sbn_block_stat| BlockStat { failing_rows: s.failing_rows as usize, first_row: if s.first_row == u64::MAX { None } else { Some(s.first_row as usize) } };
        Ok(TraceExplanation { blocks: bs.iter().map(stat).collect(), zs: zs.iter().map(stat).collect() })
    }

    /// `prove(stark, &config, trace, pi, &mut timing)` with a host-built trace: column-major already, one copy to
    /// flatten it and one PCIe transfer (0.88 GB for G1ExpStark(128)).
    pub fn prove<F, C, const D: usize>(&mut self, trace: Vec<PolynomialValues<F>>, public_inputs: &[F]) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        let (flat, pis) = self.flatten(trace, public_inputs)?;
        check(unsafe { ffi::sbn_prover_load_trace(self.raw, flat.as_ptr(), pis.as_ptr(), pis.len()) }, "sbn_prover_load_trace")?;
        self.finish::<F, C, D>()
    }

    /// (`Prover::prove` / sbn_prover_load_trace only; `prove_host_trace` and the free `prove` read the columns where they lie.)
    /// The trace as the C ABI takes it (column-major, flat) and the public inputs, as canonical u64.  The library reads
    /// num_columns * 2^degree_bits words and n_pi public inputs: the sizes are checked here, before the FFI call.
    fn flatten<F: RichField>(&self, trace: Vec<PolynomialValues<F>>, public_inputs: &[F]) -> Result<(Vec<u64>, Vec<u64>)> {
        let n = trace.first().map(|c| c.len()).unwrap_or(0);
        ensure!(trace.len() == self.n_cols, "the table has {} columns, the trace {}", self.n_cols, trace.len());
        ensure!(n == 1usize << self.degree_bits, "the prover was created for 2^{} rows, the trace has {}", self.degree_bits, n);
        ensure!(public_inputs.len() == self.n_pi, "expected {} public inputs, got {}", self.n_pi, public_inputs.len());
        let mut flat = Vec::with_capacity(trace.len() * n);
        for col in &trace {
            ensure!(col.len() == n, "ragged trace");
            flat.extend(col.values.iter().map(|x| x.to_canonical_u64()));
        }
        Ok((flat, public_inputs.iter().map(|x| x.to_canonical_u64()).collect()))
    }

    /// The column pointers of a trace as sbn_prover_prove_host_columns takes them, after the size checks of `flatten`; nothing is
    /// copied.  ASSUMPTION, unverified here (no Rust toolchain, plonky2 not vendored): `GoldilocksField` is
    /// `#[repr(transparent)]` over one `u64`, so a column's `values.as_ptr()` points at `len` u64 words.  The words may be any
    /// 64-bit representatives: the callers pass SBN_TRACE_REDUCE and the library takes them mod p on the device.
    fn column_ptrs<F: RichField>(&self, trace: &[PolynomialValues<F>]) -> Result<Vec<*const u64>> {
        let n = trace.first().map(|c| c.len()).unwrap_or(0);
        ensure!(std::mem::size_of::<F>() == 8 && std::mem::align_of::<F>() == 8, "the field element is not one u64 word");
        ensure!(trace.len() == self.n_cols, "the table has {} columns, the trace {}", self.n_cols, trace.len());
        ensure!(n == 1usize << self.degree_bits, "the prover was created for 2^{} rows, the trace has {}", self.degree_bits, n);
        ensure!(trace.iter().all(|c| c.len() == n), "ragged trace");
        Ok(trace.iter().map(|col| col.values.as_ptr() as *const u64).collect())
    }

    /// The same call with the upload INSIDE the proof (sbn_prover_prove_host_columns): the trace crosses PCIe in the commit
    /// pipeline's column chunks while earlier chunks are transformed and hashed, read from the columns where they lie -- no
    /// flattened copy, no `to_canonical_u64` pass: words >= p are reduced on the device behind the upload (SBN_TRACE_REDUCE).
    /// Same proof as `prove`; afterwards the trace is resident on the device.  (Source only, like the rest of this crate: no Rust
    /// toolchain where the library is built and tested.)
    pub fn prove_host_trace<F, C, const D: usize>(&mut self, trace: Vec<PolynomialValues<F>>, public_inputs: &[F]) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        ensure!(public_inputs.len() == self.n_pi, "expected {} public inputs, got {}", self.n_pi, public_inputs.len());
        let cols = self.column_ptrs(&trace)?;
        let pis: Vec<u64> = public_inputs.iter().map(|x| x.to_canonical_u64()).collect();
        let mut p = ptr::null_mut();
        let rc = unsafe { ffi::sbn_prover_prove_host_columns(self.raw, cols.as_ptr(), cols.len(), SBN_TRACE_REDUCE, pis.as_ptr(), pis.len(), ptr::null_mut(), &mut p) };
        drop(trace);   // the columns are read until the call returns
        check(rc, "sbn_prover_prove_host_columns")?;
        Self::take_proof::<F, C, D>(p)
    }

    /// Witness generated on the device from the instance list (`G1ExpIONative` etc. flattened to u32 limbs as
    /// include/sbn.h documents per table); no trace on the host at all.  Returns the proof; its `public_inputs` are the
    /// ones `generate_public_inputs` would have produced.
    pub fn prove_ios<F, C, const D: usize>(&mut self, ios: &[u32]) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        ensure!(self.io_words > 0, "device witness generation covers the Exp tables");
        ensure!(ios.len() == self.io_words * self.num_io, "ios must hold {} u32 words per instance x {} instances", self.io_words, self.num_io);
        let mut pi = vec![0u64; self.n_pi];
        check(unsafe { ffi::sbn_prover_generate_trace(self.raw, ios.as_ptr(), self.num_io, pi.as_mut_ptr()) }, "sbn_prover_generate_trace")?;
        self.finish::<F, C, D>()
    }

    /// Verified proving (sbn_prover_set_guard): with `Guard::Device` or `Guard::Host` every proof this prover returns has passed
    /// that verifier first; a proof it rejects is an `Err` carrying status -6 and the verifier's own reason, and the trace stays
    /// loaded, so `check_trace`, `explain_*` and `diff_witness` can name the cause.  The words of an accepted proof are those of
    /// the unguarded call.
    pub fn set_guard(&mut self, guard: Guard) -> Result<()> {
        check(unsafe { ffi::sbn_prover_set_guard(self.raw, guard.raw()) }, "sbn_prover_set_guard")
    }

    /// (proofs checked, proofs rejected, nanoseconds spent checking, device bytes of the guard) (sbn_prover_guard_stats).
    pub fn guard_stats(&self) -> Result<[u64; 4]> {
        let mut out = [0u64; 4];
        check(unsafe { ffi::sbn_prover_guard_stats(self.raw, out.as_mut_ptr()) }, "sbn_prover_guard_stats")?;
        Ok(out)
    }

    /// The shape of the reference's `G1ExpStarkyProofGenerator::run_once` (src/curves/g1/circuit.rs:187-201), which calls
    /// `prove(...)` and on the next line `verify_stark_proof(stark, inner_proof.clone(), &inner_config).unwrap()`: `prove_ios`
    /// under the device guard.  The proof that comes back has passed the verifier the consumer will run; one that does not
    /// verify is an `Err`, never a value.  The guard stays set on this prover.
    pub fn prove_ios_verified<F, C, const D: usize>(&mut self, ios: &[u32]) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        self.set_guard(Guard::Device)?;
        self.prove_ios::<F, C, D>(ios)
    }

    /// The reference's `*_msm` call shape (`test_g1_msm`, src/curves/g1/circuit.rs:459-509): `terms` holds the instance rows
    /// without their offset words (x, then exp_val), `start` the offset of instance 0, and offset[k+1] is the output of instance
    /// k; the offsets are derived on the device where the table's chains run there.  Loads the witness and returns
    /// (public inputs, the explicit instance list as `prove_ios` takes it); `prove_loaded` then proves it.
    pub fn generate_trace_chained(&mut self, terms: &[u32], start: &[u32]) -> Result<(Vec<u64>, Vec<u32>)> {
        ensure!(self.io_words > 0, "device witness generation covers the Exp tables");
        let exp_words = if self.io_words == 194 { 2 } else { 8 };
        let x_words = (self.io_words - exp_words) / 2;
        ensure!(terms.len() == (x_words + exp_words) * self.num_io, "terms must hold {} u32 words per instance x {} instances", x_words + exp_words, self.num_io);
        ensure!(start.len() == x_words, "start must hold {} u32 words", x_words);
        let mut pi = vec![0u64; self.n_pi];
        let mut ios = vec![0u32; self.io_words * self.num_io];
        check(
            unsafe { ffi::sbn_prover_generate_trace_chained(self.raw, terms.as_ptr(), self.num_io, start.as_ptr(), pi.as_mut_ptr(), ios.as_mut_ptr()) },
            "sbn_prover_generate_trace_chained",
        )?;
        Ok((pi, ios))
    }

    /// The proof of the witness the last `generate_trace_chained` (or `prove_ios`, `prove`) left on the device.
    pub fn prove_loaded<F, C, const D: usize>(&mut self) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        self.finish::<F, C, D>()
    }

    fn finish<F, C, const D: usize>(&mut self) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        let mut p = ptr::null_mut();
        check(unsafe { ffi::sbn_prover_prove(self.raw, &mut p) }, "sbn_prover_prove")?;
        Self::take_proof::<F, C, D>(p)
    }

    /// Converts and frees the library's proof object.
    fn take_proof<F, C, const D: usize>(p: *mut ffi::sbn_proof) -> Result<StarkProofWithPublicInputs<F, C, D>>
    where
        F: RichField + Extendable<D>,
        C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    {
        let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) };
        let proof = convert::proof_from_words::<F, C, D>(words);
        unsafe { ffi::sbn_proof_free(p) };
        proof
    }

    /// Which rows of the loaded trace break a constraint (sbn_prover_check_trace): what a debug build of starky's `prove` learns
    /// from `check_constraints`, for the trace the last `prove` / `prove_host_trace` / `prove_ios` of this prover left on the device.
    /// `Ok` means the check ran; the verdict is `TraceReport::ok()`.  A debugging aid, not a soundness statement (include/sbn.h).
    pub fn check_trace(&mut self, seed: u64) -> Result<TraceReport> {
        let mut raw = ffi::sbn_trace_report { struct_size: std::mem::size_of::<ffi::sbn_trace_report>() as u32, ..Default::default() };
        check(unsafe { ffi::sbn_prover_check_trace(self.raw, seed, &mut raw, ptr::null_mut()) }, "sbn_prover_check_trace")?;
        let row = |r: u64| if r == u64::MAX { None } else { Some(r as usize) };
        Ok(TraceReport {
            rows: raw.rows as usize,
            failing_rows: raw.failing_rows as usize,
            first_failing_row: row(raw.first_failing_row),
            segments: (0..raw.num_segments as usize)
                .map(|s| TraceSegment {
                    name: unsafe { CStr::from_ptr(ffi::sbn_trace_segment_name(s as i32)) }.to_string_lossy().into_owned(),
                    failing_rows: raw.seg_failing_rows[s] as usize,
                    first_row: row(raw.seg_first_row[s]),
                })
                .collect(),
        })
    }

    /// The loaded trace against the canonical witness of its instance list, cell by cell (sbn_prover_diff_witness): the witness is
    /// rebuilt on the device from `ios` (`num_io` rows in the layout `prove_ios` takes), or with `None` from the instances the
    /// loaded public inputs carry; up to `cells` (at most 65,536) differing cells are listed, main columns first.  For the trace
    /// of the reference's own `generate_trace`, loaded by `prove` / `prove_host_trace`, this names the cell where the two
    /// generators part.  `Ok` means the diff ran; the verdict is `WitnessDiff::ok()`.  The trace stays loaded, also after a refusal.
    pub fn diff_witness(&mut self, ios: Option<&[u32]>, num_io: usize, cells: usize) -> Result<WitnessDiff> {
        let mut raw = ffi::sbn_witness_diff { struct_size: std::mem::size_of::<ffi::sbn_witness_diff>() as u32, ..Default::default() };
        let mut listed = vec![ffi::sbn_witness_cell::default(); cells];
        let list_ptr = if cells == 0 { ptr::null_mut() } else { listed.as_mut_ptr() };
        let ios_ptr = ios.map_or(ptr::null(), |w| w.as_ptr());
        check(
            unsafe { ffi::sbn_prover_diff_witness(self.raw, ios_ptr, num_io, &mut raw, ptr::null_mut(), ptr::null_mut(), list_ptr, cells) },
            "sbn_prover_diff_witness",
        )?;
        listed.truncate(raw.listed as usize);
        let at = |r: u64| if r == u64::MAX { None } else { Some(r as usize) };
        Ok(WitnessDiff {
            cells: raw.cells as usize,
            main_cells: raw.main_cells as usize,
            rows: raw.rows as usize,
            columns: raw.columns as usize,
            first_row: at(raw.first_row),
            first_column: at(raw.first_column),
            pi_words: raw.pi_words as usize,
            first_pi_word: at(raw.first_pi_word),
            listed,
        })
    }

    /// Per-stage device times of the last prove() in milliseconds (sbn_prover_stage_times / sbn_prover_stage_name).
    pub fn stage_times(&self) -> Vec<(String, f32)> {
        let mut ms = [0f32; 32];
        let k = unsafe { ffi::sbn_prover_stage_times(self.raw, ms.as_mut_ptr(), 32) } as usize;
        (0..k)
            .map(|i| (unsafe { CStr::from_ptr(ffi::sbn_prover_stage_name(i as i32)) }.to_string_lossy().into_owned(), ms[i]))
            .collect()
    }
}

/// One segment of the constraint stream in a `TraceReport`: "air_head", "air_tail", "perm_lo", "perm_hi".
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct TraceSegment {
    pub name: String,
    pub failing_rows: usize,
    pub first_row: Option<usize>,
}

/// `Prover::check_trace`: the rows of the trace on which a segment of the constraints is non-zero.  Segment and row are the
/// granularity of this report; `Prover::explain_rows` names the constraint blocks a row breaks.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct TraceReport {
    pub rows: usize,
    pub failing_rows: usize,
    pub first_failing_row: Option<usize>,
    pub segments: Vec<TraceSegment>,
}

impl TraceReport {
    pub fn ok(&self) -> bool {
        self.failing_rows == 0
    }
}

/// `Prover::diff_witness`: how the loaded trace differs from the canonical witness of its instances.  The counts are exact whatever
/// the cap; `listed` holds the first differing cells in ascending (row, column) order over the main columns, the derived columns
/// only behind them -- the first listed main cell is the cause, what follows it the consequence.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct WitnessDiff {
    pub cells: usize,
    pub main_cells: usize,
    pub rows: usize,
    pub columns: usize,
    pub first_row: Option<usize>,
    pub first_column: Option<usize>,
    /// loaded public inputs that differ from those the instances determine (in practice wrong outputs)
    pub pi_words: usize,
    pub first_pi_word: Option<usize>,
    pub listed: Vec<ffi::sbn_witness_cell>,
}

impl WitnessDiff {
    pub fn ok(&self) -> bool {
        self.cells == 0 && self.pi_words == 0
    }
}

/// One block of a table's constraint stream (include/sbn.h `sbn_constraint_block`).
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct ConstraintBlock {
    pub first: usize,
    pub count: usize,
    /// 0 = air_head, 1 = air_tail
    pub segment: usize,
    /// the section name of sbn_constraint_section_name: "gadget_add", "range_check_lookup", ..
    pub section: String,
    pub instance: Option<usize>,
    pub col_first: usize,
    pub col_count: usize,
}

fn constraint_blocks_of(a: &ffi::sbn_air_desc) -> Vec<ConstraintBlock> {
    let n = unsafe { ffi::sbn_air_constraint_blocks(a, ptr::null_mut(), 0) };
    let mut raw = vec![ffi::sbn_constraint_block::default(); n];
    unsafe { ffi::sbn_air_constraint_blocks(a, raw.as_mut_ptr(), n) };
    raw.iter()
        .map(|b| ConstraintBlock {
            first: b.first as usize,
            count: b.count as usize,
            segment: b.segment as usize,
            section: unsafe { CStr::from_ptr(ffi::sbn_constraint_section_name(b.section as i32)) }.to_string_lossy().into_owned(),
            instance: if b.instance == u32::MAX { None } else { Some(b.instance as usize) },
            col_first: b.col_first as usize,
            col_count: b.col_count as usize,
        })
        .collect()
}

/// `Prover::explain_rows`: the indices (into `Prover::constraint_blocks`) of the blocks and the Z columns one row breaks.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct RowExplanation {
    pub row: usize,
    pub blocks: Vec<usize>,
    pub zs: Vec<usize>,
}

#[derive(Clone, Debug, PartialEq, Eq)]
pub struct BlockStat {
    pub failing_rows: usize,
    pub first_row: Option<usize>,
}

/// `Prover::explain_trace`: one `BlockStat` per block of `Prover::constraint_blocks` and per permutation Z column.
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct TraceExplanation {
    pub blocks: Vec<BlockStat>,
    pub zs: Vec<BlockStat>,
}

impl TraceExplanation {
    pub fn ok(&self) -> bool {
        self.blocks.iter().chain(self.zs.iter()).all(|s| s.failing_rows == 0)
    }
}

/// flags bit 0 of sbn_prover_prove_host_columns (include/sbn.h): a word >= p is taken mod p on the device instead of refused
pub const SBN_TRACE_REDUCE: u32 = 1;

impl Drop for Prover {
    fn drop(&mut self) {
        unsafe { ffi::sbn_prover_destroy(self.raw) }
    }
}

/// starky 0.1.1 `prover::prove`, signature for signature (the fork the reference pins takes the public inputs as a `Vec`,
/// which is why its call sites write `pi.try_into().unwrap()`: src/curves/g1/exp.rs:822, src/curves/g1/circuit.rs:196):
///
/// `prove::<F, C, S, D>(stark, &config, trace_poly_values, public_inputs, &mut timing) -> Result<StarkProofWithPublicInputs<F, C, D>>`
///
/// `S: Stark<F, D>` is kept so that the call sites type-check unchanged; `SbnTable` names the table for the C ABI (the
/// constraint code of `S::eval_packed_generic` lives natively on the far side, include/sbn.h).  `C::Hasher` must be
/// Poseidon -- the only hasher the reference uses (`PoseidonGoldilocksConfig`).  `timing` gets one scope for the call; the
/// per-stage device times are logged at debug level (`Prover::stage_times`).
pub fn prove<F, C, S, const D: usize>(
    stark: S,
    config: &StarkConfig,
    trace_poly_values: Vec<PolynomialValues<F>>,
    public_inputs: Vec<F>,
    timing: &mut TimingTree,
) -> Result<StarkProofWithPublicInputs<F, C, D>>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    S: Stark<F, D> + SbnTable,
{
    let n = trace_poly_values.first().map(|c| c.len()).unwrap_or(0);
    ensure!(n.is_power_of_two(), "trace height must be a power of two");
    timing.push("sbn prove (MI355X)", log::Level::Debug);
    let mut prover = Prover::new(&stark, config, n.trailing_zeros() as usize)?;
    let proof = prover.prove_host_trace::<F, C, D>(trace_poly_values, &public_inputs);   // the upload inside the trace commitment, from the columns where they lie
    for (name, ms) in prover.stage_times() {
        log::debug!("sbn stage {name}: {ms:.3} ms");
    }
    timing.pop();
    proof
}

/// starky 0.1.1 `verifier::verify_stark_proof`, signature for signature (src/curves/g1/exp.rs:826, circuit.rs:200):
/// the proof is serialised back to the library's canonical words (`convert::words_from_proof`) and checked by the
/// library's host verifier (no GPU needed).  The reference's own starky verifier can be kept instead -- then the two
/// verifiers are compared on every proof, which is the parity campaign of DESIGN.md section 6; whether it accepts hinges on
/// the recalled protocol details of DESIGN.md section 4, first of all on `FRI_VARIANT` matching the linked plonky2.
pub fn verify_stark_proof<F, C, S, const D: usize>(stark: S, proof_with_pis: StarkProofWithPublicInputs<F, C, D>, config: &StarkConfig) -> Result<()>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    S: Stark<F, D> + SbnTable,
{
    let degree_bits = proof_with_pis.proof.recover_degree_bits(config);
    let words = convert::words_from_proof::<F, C, D>(&proof_with_pis, degree_bits, config)?;
    verify_stark_proof_words(&stark, &words, config)
}

/// Several host traces in flight on one GPU (sbn_batch_prover_prove_host_columns): every unit is a trace as `prove` takes it with
/// its public inputs; one unit's upload runs beside the other contexts' kernels.  The columns are read where they lie
/// (`Prover::column_ptrs` names the layout assumption) and reduced on the device.  Proofs in unit order.
pub fn prove_host_traces<F, C, S, const D: usize>(
    stark: &S,
    config: &StarkConfig,
    degree_bits: usize,
    inflight: usize,
    traces: Vec<Vec<PolynomialValues<F>>>,
    public_inputs: &[Vec<F>],
) -> Result<Vec<StarkProofWithPublicInputs<F, C, D>>>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    S: SbnTable,
{
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let n_cols = unsafe { ffi::sbn_air_num_columns(&a) };
    let n_pi = unsafe { ffi::sbn_air_num_public_inputs(&a) };
    ensure!(traces.len() == public_inputs.len(), "one list of public inputs per trace");
    ensure!(std::mem::size_of::<F>() == 8 && std::mem::align_of::<F>() == 8, "the field element is not one u64 word");
    let mut cols: Vec<*const u64> = Vec::with_capacity(traces.len() * n_cols);
    for t in &traces {
        ensure!(t.len() == n_cols && t.iter().all(|c| c.len() == 1usize << degree_bits), "a trace does not have the table's shape");
        cols.extend(t.iter().map(|col| col.values.as_ptr() as *const u64));
    }
    ensure!(public_inputs.iter().all(|p| p.len() == n_pi), "expected {} public inputs per trace", n_pi);
    let pis: Vec<Vec<u64>> = public_inputs.iter().map(|p| p.iter().map(|x| x.to_canonical_u64()).collect()).collect();
    let pi_ptrs: Vec<*const u64> = pis.iter().map(|p| p.as_ptr()).collect();
    let mut b = ptr::null_mut();
    check(unsafe { ffi::sbn_batch_prover_create(&a, &cfg, degree_bits as u32, inflight as u32, &mut b) }, "sbn_batch_prover_create")?;
    let mut raw = vec![ptr::null_mut(); traces.len()];
    let rc = unsafe { ffi::sbn_batch_prover_prove_host_columns(b, cols.as_ptr(), n_cols, SBN_TRACE_REDUCE, pi_ptrs.as_ptr(), n_pi, traces.len(), raw.as_mut_ptr()) };
    unsafe { ffi::sbn_batch_prover_destroy(b) };
    drop(traces);   // the columns are read until the call returns
    check(rc, "sbn_batch_prover_prove_host_columns")?;
    raw.into_iter()
        .map(|p| {
            let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) };
            let proof = convert::proof_from_words::<F, C, D>(words);
            unsafe { ffi::sbn_proof_free(p) };
            proof
        })
        .collect()
}

/// Several proofs in flight on one GPU (BASELINE config 2): `units` instance lists of `num_io` instances each.
pub fn prove_batch<F, C, S, const D: usize>(stark: &S, config: &StarkConfig, degree_bits: usize, inflight: usize, ios: &[u32], units: usize) -> Result<Vec<StarkProofWithPublicInputs<F, C, D>>>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F, Hasher = PoseidonHash>,
    S: SbnTable,
{
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    ensure!(units > 0 && ios.len() % units == 0, "ios length is not a multiple of the unit count");
    let mut b = ptr::null_mut();
    check(unsafe { ffi::sbn_batch_prover_create(&a, &cfg, degree_bits as u32, inflight as u32, &mut b) }, "sbn_batch_prover_create")?;
    let mut raw = vec![ptr::null_mut(); units];
    let rc = unsafe { ffi::sbn_batch_prover_prove_ios(b, ios.as_ptr(), ios.len() / units, a.num_io as usize, units, raw.as_mut_ptr()) };
    unsafe { ffi::sbn_batch_prover_destroy(b) };
    check(rc, "sbn_batch_prover_prove_ios")?;
    raw.into_iter()
        .map(|p| {
            let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) };
            let proof = convert::proof_from_words::<F, C, D>(words);
            unsafe { ffi::sbn_proof_free(p) };
            proof
        })
        .collect()
}

/// A chained list of any length (`terms`: `count` rows of x and exp_val, `start`: the offset of instance 0; include/sbn.h, "Long
/// chained lists") proved as units of the table, the last one padded with copies of the last instance as the reference's
/// `g1_exp_circuit` pads (src/curves/g1/circuit.rs:273-277).  Returns the unit proofs as canonical words, in unit order, and the
/// last output in the word shape of `start`.
pub fn prove_msm<S: SbnTable>(stark: &S, config: &StarkConfig, degree_bits: usize, inflight: usize, terms: &[u32], count: usize, start: &[u32]) -> Result<(Vec<Vec<u64>>, Vec<u32>)> {
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let units = unsafe { ffi::sbn_msm_num_units(count, a.num_io as usize) };
    ensure!(units > 0 && terms.len() % count == 0, "terms length is not a multiple of the instance count");
    let mut b = ptr::null_mut();
    check(unsafe { ffi::sbn_batch_prover_create(&a, &cfg, degree_bits as u32, inflight as u32, &mut b) }, "sbn_batch_prover_create")?;
    let mut raw = vec![ptr::null_mut(); units];
    let mut last = vec![0u32; start.len()];
    let rc = unsafe { ffi::sbn_batch_prover_prove_msm(b, terms.as_ptr(), count, start.as_ptr(), raw.as_mut_ptr(), last.as_mut_ptr(), ptr::null_mut()) };
    unsafe { ffi::sbn_batch_prover_destroy(b) };
    check(rc, "sbn_batch_prover_prove_msm")?;
    let proofs = raw
        .into_iter()
        .map(|p| {
            let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) }.to_vec();
            unsafe { ffi::sbn_proof_free(p) };
            words
        })
        .collect();
    Ok((proofs, last))
}

/// Verifies every unit proof of `prove_msm` with the host verifier, then checks on their public inputs (the last header[5] words of
/// a proof) that the units are one chained list from `start` (`sbn_msm_check_links`; with `terms`, that x and the exponents are the
/// caller's).  Returns the last output in the word shape of `start`.
pub fn verify_msm<S: SbnTable>(stark: &S, config: &StarkConfig, proofs: &[Vec<u64>], count: usize, start: &[u32], terms: Option<&[u32]>) -> Result<Vec<u32>> {
    let a = air(stark);
    let mut pis = Vec::with_capacity(proofs.len());
    for w in proofs {
        verify_stark_proof_words(stark, w, config)?;
        ensure!(w.len() >= 12 && w[5] as usize <= w.len() - 12, "proof words truncated");
        pis.push(w[w.len() - w[5] as usize..].as_ptr());
    }
    let mut last = vec![0u32; start.len()];
    let t = terms.map_or(ptr::null(), |t| t.as_ptr());
    check(unsafe { ffi::sbn_msm_check_links(a.kind, a.num_io as usize, pis.as_ptr(), pis.len(), count, t, start.as_ptr(), last.as_mut_ptr()) }, "sbn_msm_check_links")?;
    Ok(last)
}

/// Independent scalar multiplications e_k x_k (include/sbn.h, "Scalar multiplications"; the call shape of the reference's
/// `g2_mul_by_cofactor_circuit`, src/curves/g2/circuit.rs:335-367) proved as units of a curve table: `points` holds `count` rows
/// of x words, `scalars` `count` rows of eight u32 limbs or ONE row shared by every instance (256-bit, never reduced), `offset` the
/// offset every instance carries (`None`: the curve's generator).  Returns the unit proofs as canonical words, in unit order, the
/// products in the word shape of a point and one flag per product that is the point at infinity (its words are zero).
pub fn prove_scalar_muls<S: SbnTable>(stark: &S, config: &StarkConfig, degree_bits: usize, inflight: usize, points: &[u32], count: usize, scalars: &[u32], offset: Option<&[u32]>) -> Result<(Vec<Vec<u64>>, Vec<u32>, Vec<u8>)> {
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let units = unsafe { ffi::sbn_msm_num_units(count, a.num_io as usize) };
    ensure!(units > 0 && points.len() % count == 0, "points length is not a multiple of the instance count");
    ensure!(scalars.len() == 8 || scalars.len() == 8 * count, "scalars must be one row of 8 u32 or one per instance");
    let mut b = ptr::null_mut();
    check(unsafe { ffi::sbn_batch_prover_create(&a, &cfg, degree_bits as u32, inflight as u32, &mut b) }, "sbn_batch_prover_create")?;
    let mut raw = vec![ptr::null_mut(); units];
    let mut products = vec![0u32; points.len()];
    let mut infinity = vec![0u8; count];
    let off = offset.map_or(ptr::null(), |o| o.as_ptr());
    let rc = unsafe {
        ffi::sbn_batch_prover_prove_scalar_muls(b, points.as_ptr(), scalars.as_ptr(), scalars.len() / 8, count, off, raw.as_mut_ptr(), products.as_mut_ptr(), infinity.as_mut_ptr(), ptr::null_mut())
    };
    unsafe { ffi::sbn_batch_prover_destroy(b) };
    check(rc, "sbn_batch_prover_prove_scalar_muls")?;
    let proofs = raw
        .into_iter()
        .map(|p| {
            let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) }.to_vec();
            unsafe { ffi::sbn_proof_free(p) };
            words
        })
        .collect();
    Ok((proofs, products, infinity))
}

/// Verifies every unit proof of `prove_scalar_muls` with the host verifier, then checks on their public inputs that x, exponents
/// and offset are the caller's, that the pads repeat the last instance and that every output is a point of the curve
/// (`sbn_scalar_mul_check`).  Returns the products and infinity flags recomputed from the outputs.
pub fn verify_scalar_muls<S: SbnTable>(stark: &S, config: &StarkConfig, proofs: &[Vec<u64>], points: &[u32], count: usize, scalars: &[u32], offset: Option<&[u32]>) -> Result<(Vec<u32>, Vec<u8>)> {
    let a = air(stark);
    let mut pis = Vec::with_capacity(proofs.len());
    for w in proofs {
        verify_stark_proof_words(stark, w, config)?;
        ensure!(w.len() >= 12 && w[5] as usize <= w.len() - 12, "proof words truncated");
        pis.push(w[w.len() - w[5] as usize..].as_ptr());
    }
    ensure!(scalars.len() == 8 || scalars.len() == 8 * count, "scalars must be one row of 8 u32 or one per instance");
    let mut products = vec![0u32; points.len()];
    let mut infinity = vec![0u8; count];
    let off = offset.map_or(ptr::null(), |o| o.as_ptr());
    check(
        unsafe {
            ffi::sbn_scalar_mul_check(a.kind, a.num_io as usize, pis.as_ptr(), pis.len(), count, points.as_ptr(), scalars.as_ptr(), scalars.len() / 8, off, products.as_mut_ptr(), infinity.as_mut_ptr())
        },
        "sbn_scalar_mul_check",
    )?;
    Ok((products, infinity))
}

/// Cofactor clearing on the twist (g2/circuit.rs:335-367): `prove_scalar_muls` on a `G2ExpStark` with the generator as offset and
/// the shared scalar 2p - r (`sbn_g2_cofactor`).  Returns the unit proofs, the cleared points and their infinity flags.
pub fn prove_mul_by_cofactor<S: SbnTable>(stark: &S, config: &StarkConfig, degree_bits: usize, inflight: usize, points: &[u32], count: usize) -> Result<(Vec<Vec<u64>>, Vec<u32>, Vec<u8>)> {
    let mut cofactor = [0u32; 8];
    check(unsafe { ffi::sbn_g2_cofactor(cofactor.as_mut_ptr()) }, "sbn_g2_cofactor")?;
    ensure!(air(stark).kind == ffi::SBN_AIR_G2_EXP, "cofactor clearing is a call of G2ExpStark (the twist)");
    prove_scalar_muls(stark, config, degree_bits, inflight, points, count, &cofactor, None)
}

/// A field program (include/sbn.h, "Field programs") proved as units of a field Exp table (`FqExpStark`, `Fq12ExpStark`,
/// `Fq12ExpU64Stark`): node g is instance g, its x and offset each a literal of `values` (`n_values` rows), `SBN_NODE_OUTPUT | j` for
/// the output of an earlier node, or (offset only) `SBN_NODE_ONE`; its exponent a row of `exps` (`n_exps` rows).  The list is derived
/// once on the host pool, cut into units and padded.  Returns the unit proofs as canonical words, in unit order, and the outputs
/// (`nodes.len()` rows in the word shape of a literal).
pub fn prove_program<S: SbnTable>(stark: &S, config: &StarkConfig, degree_bits: usize, inflight: usize, nodes: &[ffi::sbn_program_node], values: &[u32], n_values: usize, exps: &[u32], n_exps: usize) -> Result<(Vec<Vec<u64>>, Vec<u32>)> {
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let units = unsafe { ffi::sbn_msm_num_units(nodes.len(), a.num_io as usize) };
    ensure!(units > 0 && n_values > 0 && n_exps > 0 && values.len() % n_values == 0 && exps.len() % n_exps == 0, "no node, or values / exps are not n_values / n_exps rows");
    let mut b = ptr::null_mut();
    check(unsafe { ffi::sbn_batch_prover_create(&a, &cfg, degree_bits as u32, inflight as u32, &mut b) }, "sbn_batch_prover_create")?;
    let mut raw = vec![ptr::null_mut(); units];
    let mut outs = vec![0u32; values.len() / n_values * nodes.len()];
    let rc = unsafe { ffi::sbn_batch_prover_prove_program(b, nodes.as_ptr(), nodes.len(), values.as_ptr(), n_values, exps.as_ptr(), n_exps, raw.as_mut_ptr(), outs.as_mut_ptr(), ptr::null_mut()) };
    unsafe { ffi::sbn_batch_prover_destroy(b) };
    check(rc, "sbn_batch_prover_prove_program")?;
    let proofs = raw
        .into_iter()
        .map(|p| {
            let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) }.to_vec();
            unsafe { ffi::sbn_proof_free(p) };
            words
        })
        .collect();
    Ok((proofs, outs))
}

/// A curve program (include/sbn.h, "Curve programs") proved as units of a curve Exp table (`G1ExpStark`, `G2ExpStark`): node g is
/// instance g = offset + e x, its x a literal of `points` (`n_points` rows) or `SBN_NODE_OUTPUT | j` for the output of an earlier node,
/// its offset a literal, an earlier output or `SBN_NODE_START`, the start the library picks; its exponent a row of `exps` (`n_exps` rows
/// of eight u32 words).  The list is derived once on the host pool, cut into units and padded.  Returns the unit proofs as canonical
/// words in unit order, the values output + (-blind) (`nodes.len()` rows in the word shape of a point), their infinity flags and the
/// start candidate chosen, which `sbn_curve_program_check` takes.
pub fn prove_curve_program<S: SbnTable>(stark: &S, config: &StarkConfig, degree_bits: usize, inflight: usize, nodes: &[ffi::sbn_program_node], points: &[u32], n_points: usize, exps: &[u32], n_exps: usize) -> Result<(Vec<Vec<u64>>, Vec<u32>, Vec<u8>, u8)> {
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let units = unsafe { ffi::sbn_msm_num_units(nodes.len(), a.num_io as usize) };
    ensure!(units > 0 && n_points > 0 && n_exps > 0 && points.len() % n_points == 0 && exps.len() == 8 * n_exps, "no node, or points / exps are not n_points / n_exps rows");
    let mut b = ptr::null_mut();
    check(unsafe { ffi::sbn_batch_prover_create(&a, &cfg, degree_bits as u32, inflight as u32, &mut b) }, "sbn_batch_prover_create")?;
    let mut raw = vec![ptr::null_mut(); units];
    let mut values = vec![0u32; points.len() / n_points * nodes.len()];
    let mut infinity = vec![0u8; nodes.len()];
    let mut choice = 0u8;
    let rc = unsafe {
        ffi::sbn_batch_prover_prove_curve_program(b, nodes.as_ptr(), nodes.len(), points.as_ptr(), n_points, exps.as_ptr(), n_exps, raw.as_mut_ptr(), ptr::null_mut(), values.as_mut_ptr(), infinity.as_mut_ptr(), &mut choice, ptr::null_mut())
    };
    unsafe { ffi::sbn_batch_prover_destroy(b) };
    check(rc, "sbn_batch_prover_prove_curve_program")?;
    let proofs = raw
        .into_iter()
        .map(|p| {
            let words = unsafe { std::slice::from_raw_parts(ffi::sbn_proof_words(p), ffi::sbn_proof_num_words(p)) }.to_vec();
            unsafe { ffi::sbn_proof_free(p) };
            words
        })
        .collect();
    Ok((proofs, values, infinity, choice))
}

/// The library's host verifier on canonical proof words (what `verify_stark_proof` above ends in).
pub fn verify_stark_proof_words<S: SbnTable>(stark: &S, words: &[u64], config: &StarkConfig) -> Result<()> {
    let a = air(stark);
    let cfg = to_sbn_config(config)?;
    let bytes = unsafe { std::slice::from_raw_parts(words.as_ptr() as *const u8, words.len() * 8) };
    check(unsafe { ffi::sbn_verify(&a, &cfg, bytes.as_ptr(), bytes.len()) }, "sbn_verify")
}

/// Batch verifier on the device (sbn_verifier_*): up to `max_batch` proofs of one (table, config, degree_bits) per call, the
/// Merkle hashing and the reduction of the opened rows on the GPU.  Needs a device; `verify_stark_proof_words` is the host verifier.
pub struct Verifier {
    raw: *mut ffi::sbn_verifier,
}

impl Verifier {
    pub fn new<S: SbnTable>(stark: &S, config: &StarkConfig, degree_bits: usize, max_batch: usize) -> Result<Self> {
        let a = air(stark);
        let cfg = to_sbn_config(config)?;
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::sbn_verifier_create(&a, &cfg, degree_bits as u32, max_batch as u32, &mut raw) }, "sbn_verifier_create")?;
        Ok(Verifier { raw })
    }

    /// One `(code, reason)` per proof, in order: what `sbn_verify` returns for it (`(0, "")` = accepted).
    pub fn verify_words(&mut self, proofs: &[&[u64]]) -> Result<Vec<(i32, String)>> {
        let ptrs: Vec<*const u8> = proofs.iter().map(|w| w.as_ptr() as *const u8).collect();
        let lens: Vec<usize> = proofs.iter().map(|w| w.len() * 8).collect();
        let mut status = vec![0i32; proofs.len()];
        check(unsafe { ffi::sbn_verifier_verify(self.raw, ptrs.as_ptr(), lens.as_ptr(), proofs.len(), status.as_mut_ptr()) }, "sbn_verifier_verify")?;
        Ok((0..proofs.len())
            .map(|i| (status[i], unsafe { CStr::from_ptr(ffi::sbn_verifier_reason(self.raw, i)) }.to_string_lossy().into_owned()))
            .collect())
    }
}

impl Drop for Verifier {
    fn drop(&mut self) {
        unsafe { ffi::sbn_verifier_destroy(self.raw) }
    }
}

pub fn set_device(device: usize) -> Result<()> {
    check(unsafe { ffi::sbn_set_device(device as i32) }, "sbn_set_device")
}
