// risc0/circuit/recursion/src/prove/hal/hip.rs — the recursion circuit's HAL over the HIP
// backend, beside the reference's cuda.rs in that directory (circuit/recursion/src/prove/hal/
// cuda.rs:40-190): witness generation, accumulation and eval_check on the device through the
// r0hip_* C ABI (include/r0hip.h), and the prover constructor the crate's `recursion_prover`
// selects. Not compiled here: the image has no Rust toolchain.
use std::rc::Rc;

use anyhow::Result;
use risc0_circuit_recursion_sys::RawPreflightTrace;
use risc0_core::field::baby_bear::{BabyBearElem, BabyBearExtElem};
use risc0_sys::ffi_wrap;
use risc0_zkp::hal::{hip::{BufferImpl, HipHash}, AccumPreflight, CircuitHal};
use risc0_zkp::zkp::StepMode;
use risc0_sys::hip::{r0hip_eval_check, r0hip_recursion_accum, r0hip_recursion_witgen};
use risc0_zkp::hal::hip::{HipHal, HipHashPoseidon2, HipHashPoseidon254, HipHashSha256};
use super::{CircuitAccumulator, CircuitWitnessGenerator, RecursionProver, RecursionProverImpl};
use crate::{REGISTER_GROUP_ACCUM, REGISTER_GROUP_CTRL, REGISTER_GROUP_DATA, GLOBAL_MIX, GLOBAL_OUT};

pub struct HipRecursionCircuitHal<HS: HipHash> { _hal: Rc<HipHal<HS>> }

// Resident programs (r0hip_recursion_program_*). r0vm proves a handful of fixed programs (lift,
// join, resolve, identity_p254, ...) thousands of times, and a program's control group and its
// commitment depend only on (program, po2, suite). A HipHal that proves whole recursion proofs
// through the fused call keeps one handle per program here, beside the HAL it belongs to:
//
//     programs: RefCell<HashMap<(Digest, usize), *mut R0HipRecursionProgram>>,  // (control_id, po2)
//
// filled on first use in RecursionProverImpl::prove (prove/mod.rs:160-230), where the reference
// runs WitnessGenerator::new's host transposition (witgen.rs:57-67) and commits the control group:
//
//     let h = *programs.entry((program.control_id, po2)).or_insert_with(|| {
//         let mut h = std::ptr::null_mut();   // Program.code is Montgomery words, 23 per row
//         ffi_wrap(|| unsafe { r0hip_recursion_program_create(&mut h, HS::SUITE, po2 as u32,
//             program.code.as_ptr().cast(), program.code.len(), R0HIP_CODE_MONTGOMERY) }).unwrap();
//         h
//     });
//     r0hip_prove_recursion_program(h, wom, n_wom, cycles, n_cycles, iops, n_iops, null(), task_id, ..)
//     // on the worker: R0HipWorkerProgramJob { job: R0HipWorkerJob { kind: R0HIP_JOB_RECURSION_PROGRAM,
//     //                 recursion: {..}, .. }, program: h }, submitted as &mut pj.job
//
// With the handle, RecursionProver::prove(program, input) (prove/mod.rs:165) needs no Preflight on
// the Rust side: the library runs it natively and generates the witness from a plan kept in the handle:
//
//     r0hip_prove_recursion_program_input(h, input.as_ptr(), input.len(), null(), task_id,
//         seal, seal_cap, &mut seal_len, mix, output, output_cap, &mut n_output)
//     // on the worker: R0HipWorkerInputJob { job: R0HipWorkerJob { kind: R0HIP_JOB_RECURSION_INPUT, .. },
//     //                 program: h, h_input, n_input, h_output, output_cap, n_output: 0 }, as &mut ij.job
//
// r0hip_recursion_preflight (host only) gives wom, cycles, iops and output for a cross-check against
// Preflight::step. Programs with checked_bytes rows are refused and keep the path above.
//
// r0hip_recursion_program_info's control_id is Program::compute_control_id (program.rs:74-104) for
// the HAL's suite. The per-op path below keeps taking `ctrl` as a buffer; r0hip_recursion_program_ctrl
// gives the handle's control group for it. Drop: r0hip_recursion_program_destroy per handle, after
// the worker that was given it (destroy is refused while a job or a proof still holds the handle).

impl<HS: HipHash> CircuitWitnessGenerator<HipHal<HS>> for HipRecursionCircuitHal<HS> {
    fn generate_witness(&self, _mode: StepMode, total_cycles: u32, preflight: &RawPreflightTrace,
                        ctrl: &BufferImpl<BabyBearElem>, data: &BufferImpl<BabyBearElem>,
                        global: &BufferImpl<BabyBearElem>) -> Result<()> {
        // on the device (r0hip_recursion_witgen: step_exec, the WOM sort and scan,
        // injectWomBacks and step_verify_mem of recursion-sys ffi.cpp:57-205, generated from
        // the reference's step code); the RawPreflightTrace arrays are host memory. The
        // result is the same for every StepMode, as the reference's modes agree.
        ffi_wrap(|| unsafe {
            r0hip_recursion_witgen(ctrl.dev(), data.dev(), global.dev(), total_cycles as usize,
                preflight.wom as *const u32, preflight.num_woms as usize,
                preflight.cycles as *const u32, preflight.num_cycles as usize,
                preflight.iops as *const u32, preflight.num_iops as usize)
        })
    }
}

impl<HS: HipHash> CircuitAccumulator<HipHal<HS>> for HipRecursionCircuitHal<HS> {
    // on the device: compute, prefix product and verify of recursion-sys ffi.cpp:160-217
    // (r0hip_recursion_accum, generated from the reference step code)
    fn accumulate(&self, work_cycles: u32, total_cycles: u32, ctrl: &BufferImpl<BabyBearElem>,
                  global: &BufferImpl<BabyBearElem>, data: &BufferImpl<BabyBearElem>,
                  mix: &BufferImpl<BabyBearElem>, accum: &BufferImpl<BabyBearElem>) -> Result<()> {
        ffi_wrap(|| unsafe {
            r0hip_recursion_accum(ctrl.dev(), global.dev(), data.dev(), mix.dev(), accum.dev(),
                                  work_cycles as usize, total_cycles as usize)
        })
    }
}

impl<HS: HipHash> CircuitHal<HipHal<HS>> for HipRecursionCircuitHal<HS> {
    fn eval_check(&self, check: &BufferImpl<BabyBearElem>, groups: &[&BufferImpl<BabyBearElem>],
                  globals: &[&BufferImpl<BabyBearElem>], poly_mix: BabyBearExtElem, po2: usize, _steps: usize) {
        let g = [groups[REGISTER_GROUP_ACCUM].dev() as *const u32, groups[REGISTER_GROUP_CTRL].dev() as *const u32,
                 groups[REGISTER_GROUP_DATA].dev() as *const u32];
        let pm = poly_mix.to_u32_words();
        ffi_wrap(|| unsafe { r0hip_eval_check(c"recursion".as_ptr(), check.dev(), g.as_ptr(),
            globals[GLOBAL_MIX].dev(), globals[GLOBAL_OUT].dev(), pm.as_ptr(), po2 as u32) }).unwrap();
    }
    // CircuitHal's preflight-driven accumulate: the recursion prover never calls it (it runs
    // CircuitAccumulator::accumulate above); the reference's CUDA HAL leaves it unimplemented
    // too (circuit/recursion/src/prove/hal/cuda.rs:174-185)
    fn accumulate(&self, _preflight: &AccumPreflight, _ctrl: &BufferImpl<BabyBearElem>, _io: &BufferImpl<BabyBearElem>,
                  _data: &BufferImpl<BabyBearElem>, _mix: &BufferImpl<BabyBearElem>, _accum: &BufferImpl<BabyBearElem>,
                  _steps: usize) {
        unimplemented!("the recursion prover accumulates through CircuitAccumulator")
    }
}

pub(crate) fn recursion_prover(hashfn: &str) -> Result<Box<dyn RecursionProver>> {
    macro_rules! with { ($hs:ty) => {{
        let hal = Rc::new(HipHal::<$hs>::new());
        let circuit_hal = Rc::new(HipRecursionCircuitHal { _hal: hal.clone() });
        Ok(Box::new(RecursionProverImpl::new(hal, circuit_hal)) as Box<dyn RecursionProver>)
    }}}
    match hashfn {
        "poseidon2" => with!(HipHashPoseidon2),
        "poseidon_254" => with!(HipHashPoseidon254),
        "sha-256" => with!(HipHashSha256),
        _ => anyhow::bail!("Unsupported hashfn: {hashfn}"),
    }
}
