//! Enums and `repr(C)` structs of the boundary — field for field those bindgen emits for the reference
//! (backends/tfhe-cuda-backend/src/bindings.rs: PBS_* at :115-123, the integer / keyswitch / zk enums, CudaLweKeyswitchKeyParamsFFI :129-134,
//! CudaStreamsFFI :330-334, CudaRadixCiphertextFFI :348-355, CudaLweBootstrapKeyParamsFFI :506-515);
//! C side: include/tfhe_hip_backend.h.
use crate::ffi;

pub const PBS_TYPE_MULTI_BIT: PBS_TYPE = 0;
pub const PBS_TYPE_CLASSICAL: PBS_TYPE = 1;
pub type PBS_TYPE = ffi::c_uint;
pub const PBS_VARIANT_DEFAULT: PBS_VARIANT = 0;
pub const PBS_VARIANT_CG: PBS_VARIANT = 1;
pub const PBS_VARIANT_TBC: PBS_VARIANT = 2;
pub type PBS_VARIANT = ffi::c_uint;
pub const PBS_MS_REDUCTION_T_NO_REDUCTION: PBS_MS_REDUCTION_T = 0;
pub const PBS_MS_REDUCTION_T_CENTERED: PBS_MS_REDUCTION_T = 1;
pub type PBS_MS_REDUCTION_T = ffi::c_uint;
pub const SHIFT_OR_ROTATE_TYPE_LEFT_SHIFT: SHIFT_OR_ROTATE_TYPE = 0;
pub const SHIFT_OR_ROTATE_TYPE_RIGHT_SHIFT: SHIFT_OR_ROTATE_TYPE = 1;
pub const SHIFT_OR_ROTATE_TYPE_LEFT_ROTATE: SHIFT_OR_ROTATE_TYPE = 2;
pub const SHIFT_OR_ROTATE_TYPE_RIGHT_ROTATE: SHIFT_OR_ROTATE_TYPE = 3;
pub type SHIFT_OR_ROTATE_TYPE = ffi::c_uint;
pub const BITOP_TYPE_BITAND: BITOP_TYPE = 0;
pub const BITOP_TYPE_BITOR: BITOP_TYPE = 1;
pub const BITOP_TYPE_BITXOR: BITOP_TYPE = 2;
pub const BITOP_TYPE_SCALAR_BITAND: BITOP_TYPE = 3;
pub const BITOP_TYPE_SCALAR_BITOR: BITOP_TYPE = 4;
pub const BITOP_TYPE_SCALAR_BITXOR: BITOP_TYPE = 5;
pub type BITOP_TYPE = ffi::c_uint;
pub const COMPARISON_TYPE_EQ: COMPARISON_TYPE = 0;
pub const COMPARISON_TYPE_NE: COMPARISON_TYPE = 1;
pub const COMPARISON_TYPE_GT: COMPARISON_TYPE = 2;
pub const COMPARISON_TYPE_GE: COMPARISON_TYPE = 3;
pub const COMPARISON_TYPE_LT: COMPARISON_TYPE = 4;
pub const COMPARISON_TYPE_LE: COMPARISON_TYPE = 5;
pub const COMPARISON_TYPE_MAX: COMPARISON_TYPE = 6;
pub const COMPARISON_TYPE_MIN: COMPARISON_TYPE = 7;
pub type COMPARISON_TYPE = ffi::c_uint;
pub const KS_TYPE_BIG_TO_SMALL: KS_TYPE = 0;
pub const KS_TYPE_SMALL_TO_BIG: KS_TYPE = 1;
pub type KS_TYPE = ffi::c_uint;
pub const EXPAND_KIND_NO_CASTING: EXPAND_KIND = 0;
pub const EXPAND_KIND_CASTING: EXPAND_KIND = 1;
pub const EXPAND_KIND_SANITY_CHECK: EXPAND_KIND = 2;
pub type EXPAND_KIND = ffi::c_uint;
pub const RERAND_MODE_RERAND_WITH_KS: RERAND_MODE = 0;
pub const RERAND_MODE_RERAND_WITHOUT_KS: RERAND_MODE = 1;
pub type RERAND_MODE = ffi::c_uint;
pub const Direction_Trailing: Direction = 0;
pub const Direction_Leading: Direction = 1;
pub type Direction = ffi::c_uint;
pub const BitValue_Zero: BitValue = 0;
pub const BitValue_One: BitValue = 1;
pub type BitValue = ffi::c_uint;

#[repr(C)]
#[derive(Debug, Copy, Clone)]
pub struct CudaStreamsFFI {
    pub streams: *const *mut ffi::c_void,
    pub gpu_indexes: *const u32,
    pub gpu_count: u32,
}

#[repr(C)]
#[derive(Debug, Copy, Clone)]
pub struct CudaRadixCiphertextFFI {
    pub ptr: *mut ffi::c_void,
    pub degrees: *mut u64,
    pub noise_levels: *mut u64,
    pub num_radix_blocks: u32,
    pub max_num_radix_blocks: u32,
    pub lwe_dimension: u32,
}

#[repr(C)]
#[derive(Debug, Copy, Clone)]
pub struct CudaLweBootstrapKeyParamsFFI {
    pub input_lwe_dimension: u32,
    pub glwe_dimension: u32,
    pub polynomial_size: u32,
    pub base_log: u32,
    pub level_count: u32,
    pub big_lwe_dimension: u32,
    pub pbs_type: u32,
    pub grouping_factor: u32,
}

#[repr(C)]
#[derive(Debug, Copy, Clone)]
pub struct CudaLweKeyswitchKeyParamsFFI {
    pub input_lwe_dimension: u32,
    pub output_lwe_dimension: u32,
    pub base_log: u32,
    pub level_count: u32,
}

const _: () = {
    ["Size of CudaStreamsFFI"][::std::mem::size_of::<CudaStreamsFFI>() - 24usize];
    ["Size of CudaRadixCiphertextFFI"][::std::mem::size_of::<CudaRadixCiphertextFFI>() - 40usize];
    ["Size of CudaLweBootstrapKeyParamsFFI"][::std::mem::size_of::<CudaLweBootstrapKeyParamsFFI>() - 32usize];
    ["Size of CudaLweKeyswitchKeyParamsFFI"][::std::mem::size_of::<CudaLweKeyswitchKeyParamsFFI>() - 16usize];
};
