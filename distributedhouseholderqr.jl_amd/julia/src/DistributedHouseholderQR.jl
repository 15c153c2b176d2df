# DistributedHouseholderQR.jl -- drop-in replacement module: same names and semantics as
# jwscook/DistributedHouseholderQR.jl (src/DistributedHouseholderQR.jl), with the hot path running in
# libdhqr.so (hand-written HIP for MI355X/gfx950) through `ccall`.  No AMDGPU.jl, no CUDA.jl, no
# rocSOLVER.
#
# This file is the `src/` of a Julia PACKAGE with the reference's name and uuid (../Project.toml; deps LinearAlgebra,
# Distributed, DistributedArrays, SharedArrays like the reference's Project.toml:1-13), so that the reference's own
# tests load it the way they load the reference: `using DistributedHouseholderQR` on the master, `addprocs(np,
# exeflags=["--proj=@.", ...])`, `@everywhere using DistributedHouseholderQR` (test/runtests.jl:8-9,32).  Run them with
#   cd distributedhouseholderqr.jl_amd/julia && julia --project=@. -t 8 /root/reference/test/runtests.jl 2
# (the package's own ../test/runtests.jl restates the same acceptance checks without the reference's benchmarking deps).
#
# STATUS: written against include/dhqr.h and reviewed by hand; NOT executed -- there is no Julia
# toolchain in the build image or on the GPU box.  The identical C entry points are exercised by
# the Python ctypes binding (distributedhouseholderqr.jl_amd/_lib.py, tests/); tests/test_abi.py checks the package
# layout, that every ccall names a declared symbol with the prototype's arity, that every method is defined at module
# top level (no definition hidden behind a hook nobody calls) and that every function has a caller or is API.
#
#   reference                                 this module
#   qr!(A)                      src:311-315   qr!(A; nb=default_nb(A))      -> dhqr_qr_f64
#   H \ b                       src:317-321   \(H, b)                       -> dhqr_ldiv_f64
#   H \ B (B a Matrix)          (new)         \(H, B)                       -> dhqr_ldiv_batched_nrhs_f64 / _f32 / _c64
#   householder!(A, α)          src:113       householder!(A, α; nb=...)    -> dhqr_qr_f64
#   solve_householder!(b, H, α) src:284-294   solve_householder!(b, H, α)   -> dhqr_ldiv_f64
#   partialdot(a, b, is, T)     src:42-49     partialdot(a, b, is, Float64) -> dhqr_partialdot_host_f64 (KAT hook)
#   DistributedHouseholderQRStruct src:296-309  same fields A, α
#   ComplexF64 methods (src:9, 51-59, 171-196; test/runtests.jl:43, test/partialdot.jl) dispatch on the
#   element type exactly like the reference: qr!/householder! -> dhqr_qr_c64, \ / solve_householder!
#   -> dhqr_ldiv_c64, partialdot(a, b, is, ComplexF64) -> dhqr_partialdot_host_c64.  A Ptr{ComplexF64}
#   is the interleaved (re, im) `double *` of include/dhqr.h.
#
#   qr!(A; ndev=8)              (new)         one process, `ndev` GPUs        -> dhqr_mg_qr_f64 / dhqr_mg_ldiv_f64
#   qr!(A::DArray)              src:115-120   one Julia worker per GPU        -> dhqr_comm_create_rank + dhqr_cs_qr_darray_f64
#   qr!(A::DArray) \ b          src:317-321   the same workers (src:226-230, 256-270) -> dhqr_cs_ldiv_darray_f64 / _c64
#     householder!(A::DArray,α) src:115-120   (owners visited sequentially, every reflector sent to every process with
#     `@spawnat` src:141-143, α::SharedArray src:301-304) becomes ONE collective call per worker: the library converts
#     the DistributedArrays layout (one contiguous column block per worker) to block-cyclic columns, factors with one
#     RCCL broadcast per 128-column panel, converts back, and returns the replicated α.  The only thing Julia ships
#     between the workers is the 128-byte RCCL unique id (Distributed.jl remotecall), like an MPI bootstrap.
module DistributedHouseholderQR

using LinearAlgebra
using Distributed, DistributedArrays, SharedArrays   # src:3 -- the DArray methods and the SharedArray α (src:301-304)

const libdhqr = get(ENV, "DHQR_LIB", joinpath(@__DIR__, "..", "..", "libdhqr.so"))
const DHQR_NB = 128

struct DHQRError <: Exception
  code::Int32
  msg::String
end

function check(rc::Int32)
  rc == 0 && return nothing
  msg = unsafe_string(ccall((:dhqr_last_error, libdhqr), Cstring, ()))
  throw(DHQRError(rc, msg))
end

# one context per (process, GPU): keyed by the device, created lazily, destroyed at exit.  (A master that has factored
# on GPU 0 and is later used as worker rank i of a DArray factorisation gets a context on GPU i, not the cached one.)
const _ctx = Dict{Int, Ptr{Cvoid}}()
function context(device::Integer=0)
  get!(_ctx, Int(device)) do
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dhqr_create, libdhqr), Int32, (Ref{Ptr{Cvoid}}, Int32), h, Int32(device)))
    hd = h[]
    atexit(() -> ccall((:dhqr_destroy, libdhqr), Int32, (Ptr{Cvoid},), hd))
    hd
  end
end

struct DistributedHouseholderQRStruct{T1, T2}   # src:296-299
  A::T1
  α::T2
end
DistributedHouseholderQRStruct(A) = DistributedHouseholderQRStruct(A, zeros(eltype(A), size(A, 2)))  # src:306-309
# src:301-304: a DArray factorisation keeps α in shared memory, visible to the master and to every worker of the host
DistributedHouseholderQRStruct(A::DArray) = DistributedHouseholderQRStruct(A, SharedArray(zeros(eltype(A), size(A, 2))))

# householder!(A, α) -- src:113.  In place on A (column-major Matrix{Float64}), fills α.
# nb = 0 runs the reference's unblocked algorithm verbatim on the GPU; nb = 128 the blocked path (the default above 480 rows).
default_nb(A::StridedMatrix{Float64}) = size(A, 1) <= 480 ? 0 : DHQR_NB   # (short matrices: the unblocked passes finish first)
function householder!(A::StridedMatrix{Float64}, α::Vector{Float64}; nb::Integer=default_nb(A))
  m, n = size(A)
  stride(A, 1) == 1 || throw(ArgumentError("column-major storage required"))
  check(ccall((:dhqr_qr_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int32),
              context(), A, m, n, stride(A, 2), α, Int32(nb)))
  return (A, α)
end

function qr!(A::StridedMatrix{Float64}; nb::Integer=default_nb(A))   # src:311-315
  H = DistributedHouseholderQRStruct(A)
  householder!(H.A, H.α; nb=nb)
  return H
end

# solve_householder!(b, H, α) -- src:284-294: b <- Q'b, back substitution, returns b[1:n].
# (The device performs both phases on its own copy; b[1:n] is overwritten with the solution so
# the caller observes the same values the reference leaves in b[1:n].)
function solve_householder!(b::Vector{Float64}, H::StridedMatrix{Float64}, α::Vector{Float64})
  m, n = size(H)
  x = Vector{Float64}(undef, n)
  check(ccall((:dhqr_ldiv_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              context(), H, m, n, stride(H, 2), α, b, x))
  b[1:n] .= x
  return x
end

function LinearAlgebra.:(\)(H::DistributedHouseholderQRStruct, b::AbstractVector)   # src:317-321
  s = Vector{eltype(H.A)}(b)        # the reference copies b into a SharedArray (src:318)
  return solve_householder!(s, H.A, H.α)
end

# ---- Float32 methods ---------------------------------------------------------------------------
# The reference's qr! and `\` are generic over the element type (src:42-49, 306-321).  Up to 64 x 32 the library runs native
# Float32 kernels (float storage, double sums); every other shape is widened on the device, runs the Float64 route chosen by
# nb and is rounded back: float32(f64_route(float64(A))).  Float32 crosses PCIe.  `H \ b` is the generic method above.
default_nb(A::StridedMatrix{Float32}) = size(A, 1) <= 480 ? 0 : DHQR_NB
function householder!(A::StridedMatrix{Float32}, α::Vector{Float32}; nb::Integer=default_nb(A))
  m, n = size(A)
  stride(A, 1) == 1 || throw(ArgumentError("column-major storage required"))
  check(ccall((:dhqr_qr_f32, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int32),
              context(), A, m, n, stride(A, 2), α, Int32(nb)))
  return (A, α)
end

function qr!(A::StridedMatrix{Float32}; nb::Integer=default_nb(A))   # src:311-315
  H = DistributedHouseholderQRStruct(A)
  householder!(H.A, H.α; nb=nb)
  return H
end

function solve_householder!(b::Vector{Float32}, H::StridedMatrix{Float32}, α::Vector{Float32})   # src:284-294
  m, n = size(H)
  x = Vector{Float32}(undef, n)
  check(ccall((:dhqr_ldiv_f32, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              context(), H, m, n, stride(H, 2), α, b, x))
  b[1:n] .= x
  return x
end

# ---- H \ B for a matrix of right-hand sides ----------------------------------------------------
# Every column of B against the same factor in ONE call (a batch of 1 of dhqr_ldiv_batched_nrhs_*): up to 64 x 32 the
# factor is read once and the columns walk past it; beyond, the library runs one existing solve per column.  B is not
# modified; X is n x nrhs.  Column r of X has the bits of the BATCHED single-column entry point (batch = 1) on B[:, r]; for a
# Float64 factor of at most 64 x 32 that is the wave kernel, and H \ B[:, r] (dhqr_ldiv_f64: the one-workgroup kernel) may
# differ from it in the last bits.
function LinearAlgebra.:(\)(H::DistributedHouseholderQRStruct{<:StridedMatrix{Float64}}, B::Matrix{Float64})
  m, n = size(H.A)
  size(B, 1) == m || throw(DimensionMismatch("B has $(size(B, 1)) rows, the factor $m"))
  nrhs = size(B, 2)
  X = Matrix{Float64}(undef, n, nrhs)
  check(ccall((:dhqr_ldiv_batched_nrhs_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int64, Int64,
               Ptr{Float64}, Int64, Int64, Int64),
              context(), H.A, m, n, stride(H.A, 2), max(stride(H.A, 2) * (n - 1) + m, 1), H.α, max(n, 1),
              B, nrhs, max(m, 1), max(m * nrhs, 1), X, max(n, 1), max(n * nrhs, 1), 1))
  return X
end

function LinearAlgebra.:(\)(H::DistributedHouseholderQRStruct{<:StridedMatrix{Float32}}, B::Matrix{Float32})
  m, n = size(H.A)
  size(B, 1) == m || throw(DimensionMismatch("B has $(size(B, 1)) rows, the factor $m"))
  nrhs = size(B, 2)
  X = Matrix{Float32}(undef, n, nrhs)
  check(ccall((:dhqr_ldiv_batched_nrhs_f32, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Int64, Int64,
               Ptr{Float32}, Int64, Int64, Int64),
              context(), H.A, m, n, stride(H.A, 2), max(stride(H.A, 2) * (n - 1) + m, 1), H.α, max(n, 1),
              B, nrhs, max(m, 1), max(m * nrhs, 1), X, max(n, 1), max(n * nrhs, 1), 1))
  return X
end

# ComplexF64 (a Ptr{ComplexF64} is the library's interleaved (re, im) `double *`; leading dimensions and strides count
# complex elements): column r of X has the bits of dhqr_ldiv_batched_c64 (batch = 1) on B[:, r]
function LinearAlgebra.:(\)(H::DistributedHouseholderQRStruct{<:StridedMatrix{ComplexF64}}, B::Matrix{ComplexF64})
  m, n = size(H.A)
  size(B, 1) == m || throw(DimensionMismatch("B has $(size(B, 1)) rows, the factor $m"))
  nrhs = size(B, 2)
  X = Matrix{ComplexF64}(undef, n, nrhs)
  check(ccall((:dhqr_ldiv_batched_nrhs_c64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Int64, Int64, Int64, Ptr{ComplexF64}, Int64, Ptr{ComplexF64}, Int64, Int64, Int64,
               Ptr{ComplexF64}, Int64, Int64, Int64),
              context(), H.A, m, n, stride(H.A, 2), max(stride(H.A, 2) * (n - 1) + m, 1), H.α, max(n, 1),
              B, nrhs, max(m, 1), max(m * nrhs, 1), X, max(n, 1), max(n * nrhs, 1), 1))
  return X
end

# ---- ComplexF64 methods ------------------------------------------------------------------------
# nb = 64 (default for n >= 256): panels of 64 complex reflectors, trailing update on the FP64 MFMA kernels through the
# real 2 x 2 embedding; nb = 0: the reference's unblocked order (src:171-196).  Same factorisation either way.
# Up to 128 rows (the reference's first test shape, 110 x 100) qr! and \ are ONE single-workgroup launch each on the
# library's pinned staging buffer, whatever nb (dhqr.h, the ComplexF64 section).
const DHQR_ZNB = 64
function householder!(A::StridedMatrix{ComplexF64}, α::Vector{ComplexF64}; nb::Integer=(size(A, 2) >= 256 ? DHQR_ZNB : 0))
  (nb == 0 || nb == DHQR_ZNB) || throw(ArgumentError("ComplexF64: nb must be 0 (unblocked) or $(DHQR_ZNB) (blocked)"))
  m, n = size(A)
  stride(A, 1) == 1 || throw(ArgumentError("column-major storage required"))
  check(ccall((:dhqr_qr_c64_nb, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Int64, Int64, Ptr{ComplexF64}, Int32),
              context(), A, m, n, stride(A, 2), α, Int32(nb)))
  return (A, α)
end

function qr!(A::StridedMatrix{ComplexF64}; nb::Integer=(size(A, 2) >= 256 ? DHQR_ZNB : 0))   # src:311-315
  H = DistributedHouseholderQRStruct(A)
  householder!(H.A, H.α; nb=nb)
  return H
end

function solve_householder!(b::Vector{ComplexF64}, H::StridedMatrix{ComplexF64}, α::Vector{ComplexF64})
  m, n = size(H)
  x = Vector{ComplexF64}(undef, n)
  check(ccall((:dhqr_ldiv_c64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Int64, Int64, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
              context(), H, m, n, stride(H, 2), α, b, x))
  b[1:n] .= x
  return x
end

# partialdot(a, b, is, ::Type{<:Complex}) -- src:51-59: sum conj(a[i]) b[i]; the function
# test/partialdot.jl:12-20 checks against dot(a[i:end], b[i:end]).
function partialdot(a::Vector{ComplexF64}, b::Vector{ComplexF64}, is::UnitRange{Int}, ::Type{ComplexF64})
  out = Ref{ComplexF64}(0.0 + 0.0im)
  check(ccall((:dhqr_partialdot_host_c64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}, Int64, Int64, Ref{ComplexF64}),
              context(), a, b, first(is) - 1, last(is), out))
  return out[]
end

# partialdot(a, b, is, ::Type{<:Real}) -- src:42-49 (test/partialdot.jl:18).  Reduced on the device with the
# same wavefront-shuffle + LDS tree the factor kernels use (KAT hook).
function partialdot(a::Vector{Float64}, b::Vector{Float64}, is::UnitRange{Int}, ::Type{Float64})
  out = Ref{Float64}(0.0)
  check(ccall((:dhqr_partialdot_host_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ref{Float64}),
              context(), a, b, first(is) - 1, last(is), out))     # 1-based inclusive -> 0-based half-open
  return out[]
end

# ---- several GPUs, ONE process: qr!(A; ndev) ---------------------------------------------------------------
# The library runs one host thread + one RCCL rank per device (include/dhqr.h, "single-process handle").
const _mg = Dict{Int, Ptr{Cvoid}}()
function multigpu(ndev::Integer)
  get!(_mg, Int(ndev)) do
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dhqr_mg_create, libdhqr), Int32, (Ref{Ptr{Cvoid}}, Ptr{Int32}, Int32), h, C_NULL, Int32(ndev)))
    atexit(() -> ccall((:dhqr_mg_destroy, libdhqr), Int32, (Ptr{Cvoid},), h[]))
    h[]
  end
end

function householder!(A::StridedMatrix{Float64}, α::Vector{Float64}, ndev::Integer)
  m, n = size(A)
  stride(A, 1) == 1 || throw(ArgumentError("column-major storage required"))
  check(ccall((:dhqr_mg_qr_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}),
              multigpu(ndev), A, m, n, stride(A, 2), α))
  return (A, α)
end

# ComplexF64 over `ndev` GPUs: cyclic blocks of 64 columns (dhqr_mg_qr_c64); `\` of the result is the single-GPU
# ComplexF64 solve (the factored matrix is back on the host in the reference's format).
function householder!(A::StridedMatrix{ComplexF64}, α::Vector{ComplexF64}, ndev::Integer)
  m, n = size(A)
  stride(A, 1) == 1 || throw(ArgumentError("column-major storage required"))
  check(ccall((:dhqr_mg_qr_c64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Int64, Int64, Ptr{ComplexF64}),
              multigpu(ndev), A, m, n, stride(A, 2), α))
  return (A, α)
end

function qr!(A::StridedMatrix{ComplexF64}, ndev::Integer)
  H = DistributedHouseholderQRStruct(A)
  householder!(H.A, H.α, ndev)
  return H
end

function qr!(A::StridedMatrix{Float64}, ndev::Integer)   # qr!(A, 8): the 8 GPUs of the node
  H = DistributedHouseholderQRStruct(A)
  householder!(H.A, H.α, ndev)
  return H
end

function solve_householder!(b::Vector{Float64}, H::StridedMatrix{Float64}, α::Vector{Float64}, ndev::Integer)
  m, n = size(H)
  x = Vector{Float64}(undef, n)
  check(ccall((:dhqr_mg_ldiv_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              multigpu(ndev), H, m, n, stride(H, 2), α, b, x))
  b[1:n] .= x
  return x
end

# ---- tall-skinny matrices, ROWS split over the GPUs of one process (BASELINE configs[4]; the reference cannot split
# rows, src:33): qr!(A, ndev; split=:rows).  Same factor format; per panel the partial Gram matrices and the V'C partial
# dots are all-reduced over the devices (include/dhqr.h, dhqr_mg_rs_*).
function householder!(A::StridedMatrix{Float64}, α::Vector{Float64}, ndev::Integer, split::Symbol)
  split === :rows || return householder!(A, α, ndev)
  m, n = size(A)
  stride(A, 1) == 1 || throw(ArgumentError("column-major storage required"))
  g = multigpu(ndev)
  check(ccall((:dhqr_mg_rs_alloc_f64, libdhqr), Int32, (Ptr{Cvoid}, Int64, Int64), g, m, n))
  check(ccall((:dhqr_mg_rs_transfer_f64, libdhqr), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int32),
              g, A, stride(A, 2), C_NULL, Int32(1)))                                    # upload
  check(ccall((:dhqr_mg_rs_factor_f64, libdhqr), Int32, (Ptr{Cvoid},), g))
  check(ccall((:dhqr_mg_rs_transfer_f64, libdhqr), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int32),
              g, A, stride(A, 2), α, Int32(0)))                                        # download: factor + α
  return (A, α)
end

function qr!(A::StridedMatrix{Float64}, ndev::Integer, split::Symbol)   # qr!(A, 8, :rows)
  H = DistributedHouseholderQRStruct(A)
  householder!(H.A, H.α, ndev, split)
  return H
end

"`H \\ b` on the row-split factor that is still resident on the devices (right after qr!(A, ndev, :rows))"
function solve_rowsplit(b::Vector{Float64}, n::Integer, ndev::Integer)
  x = Vector{Float64}(undef, n)
  check(ccall((:dhqr_mg_rs_solve_f64, libdhqr), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), multigpu(ndev), b, x))
  return x
end

# ---- one Julia worker per GPU: the reference's own calling convention, qr!(A::DArray) (src:115-120, 311-315;
# test/runtests.jl:71-78).  Written against DistributedArrays' API (procs(A), localpart(A), size(A)); the package is
# loaded by the caller exactly as with the reference.  `devices[i]` is the HIP device of the i-th worker of A.
const _comm = Ref{Ptr{Cvoid}}(C_NULL)
const _comm_key = Ref{Any}(nothing)   # (worker pids, devices) the cached communicator of this worker was built for

"RCCL unique id (128 bytes): created on ONE worker, shipped to the others by the caller"
function comm_unique_id()
  id = zeros(UInt8, 128)
  check(ccall((:dhqr_comm_unique_id, libdhqr), Int32, (Ptr{UInt8},), id))
  return id
end

"does this worker already hold a communicator for `key` = (worker pids, devices)?  (qr! is called repeatedly, e.g. under
@benchmark, test/runtests.jl:84: the RCCL bootstrap -- two ncclCommInitRank and the broadcast trial -- runs once per key)"
comm_cached(key) = _comm[] != C_NULL && _comm_key[] == key

"destroy this worker's communicator (also registered with atexit)"
function comm_free()
  if _comm[] != C_NULL
    ccall((:dhqr_comm_destroy, libdhqr), Int32, (Ptr{Cvoid},), _comm[])
    _comm[] = C_NULL
    _comm_key[] = nothing
  end
  return nothing
end

"collective over the workers: bind this worker (rank `rank` of `nranks`, 0-based) to GPU `device`; replaces (and
destroys) a communicator built for another set of workers / devices"
function comm_init(id::Vector{UInt8}, nranks::Integer, rank::Integer, device::Integer, key=nothing)
  first_time = _comm_key[] === nothing && _comm[] == C_NULL
  comm_free()
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:dhqr_comm_create_rank, libdhqr), Int32,
              (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}),
              h, context(device), Int32(nranks), Int32(rank), id))
  _comm[] = h[]
  _comm_key[] = key
  first_time && atexit(comm_free)
  return nothing
end

"this worker's part of householder!(A::DArray, α): `Al` is its contiguous column block (localpart), m x n the global size"
function householder_local!(Al::StridedMatrix{Float64}, m::Integer, n::Integer, α::Vector{Float64})
  check(ccall((:dhqr_cs_qr_darray_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}),
              _comm[], Al, m, n, max(stride(Al, 2), m), α))
  return α
end
function householder_local!(Al::StridedMatrix{ComplexF64}, m::Integer, n::Integer, α::Vector{ComplexF64})
  check(ccall((:dhqr_cs_qr_darray_c64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Int64, Int64, Ptr{ComplexF64}),
              _comm[], Al, m, n, max(stride(Al, 2), m), α))
  return α
end

"this worker's part of `qrA \\ b` for a DArray factorisation (src:226-230, 256-270): `Al` is its contiguous block of the
FACTORED matrix, α the replicated diagonal of R, b the right-hand side (m, the same on every worker); returns x (n)"
function solve_local(Al::StridedMatrix{Float64}, m::Integer, n::Integer, α::Vector{Float64}, b::Vector{Float64})
  x = Vector{Float64}(undef, n)
  check(ccall((:dhqr_cs_ldiv_darray_f64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
              _comm[], Al, m, n, max(stride(Al, 2), m), α, b, x))
  return x
end
function solve_local(Al::StridedMatrix{ComplexF64}, m::Integer, n::Integer, α::Vector{ComplexF64}, b::Vector{ComplexF64})
  x = Vector{ComplexF64}(undef, n)
  check(ccall((:dhqr_cs_ldiv_darray_c64, libdhqr), Int32,
              (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Int64, Int64, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
              _comm[], Al, m, n, max(stride(Al, 2), m), α, b, x))
  return x
end

"devices the cached communicator of this worker was built with for the workers `ws` (nothing: no such communicator)"
comm_devices(ws) = (_comm[] != C_NULL && _comm_key[] !== nothing && _comm_key[][1] == ws) ? _comm_key[][2] : nothing

"GPU of the i-th worker when the caller names none: worker i -> device i-1; with fewer GPUs than workers (the reference's
own test starts two workers whatever the machine, test/runtests.jl:4,9) the workers share the GPUs round robin and the
collectives travel through Julia (`comm_init_callbacks`) -- RCCL cannot put two ranks on one device"
function default_devices(ws)
  nd = remotecall_fetch(device_count, ws[1])
  nd >= 1 || throw(ArgumentError("no GPU visible on worker $(ws[1])"))
  return [(i - 1) % nd for i in 1:length(ws)]
end

# ---- the CALLBACK transport (include/dhqr.h: dhqr_comm_create_callbacks) carried by Distributed.jl.  Every worker owns a
# mailbox (a RemoteChannel on itself); a message is (source rank, bytes).  The library calls back into Julia from inside
# dhqr_cs_* with a DEVICE pointer and the stream already synchronised; the callback copies through host memory
# (hipMemcpy of the HIP runtime the library is linked against) and returns when the data is visible to the device.
# The SPMD program issues its collectives in the same order on every rank, but a fast rank may already have sent its
# message of the NEXT collective: what arrives from a source other than the awaited one is parked per source.
const libhip = get(ENV, "DHQR_HIP_LIB", "libamdhip64.so")
mutable struct CallbackState
  boxes::Vector{RemoteChannel{Channel{Tuple{Int, Vector{UInt8}}}}}
  np::Int
  rank::Int
  parked::Vector{Vector{Vector{UInt8}}}
end
const _cb = Ref{Union{Nothing, CallbackState}}(nothing)

"this worker's mailbox (created on the worker, shipped to the others by the master)"
mailbox_create() = RemoteChannel(() -> Channel{Tuple{Int, Vector{UInt8}}}(1024), myid())

function hip_copy(dst::Ptr{Cvoid}, src::Ptr{Cvoid}, bytes::Integer, kind::Integer)   # 1: host -> device, 2: device -> host
  rc = ccall((:hipMemcpy, libhip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), dst, src, Csize_t(bytes), Cint(kind))
  rc == 0 || error("hipMemcpy failed with code $rc")
  return nothing
end

"next message from rank `src` (0-based) in this worker's mailbox"
function mailbox_recv(st::CallbackState, src::Integer)
  q = st.parked[src + 1]
  while isempty(q)
    from, bytes = take!(st.boxes[st.rank + 1])
    push!(st.parked[from + 1], bytes)
  end
  return popfirst!(q)
end

function cb_bcast(user::Ptr{Cvoid}, dbuf::Ptr{Cvoid}, bytes::Int64, root::Int32, stream::Ptr{Cvoid})::Int32
  try
    st = _cb[]::CallbackState
    if st.rank == root
      buf = Vector{UInt8}(undef, bytes)
      GC.@preserve buf hip_copy(Ptr{Cvoid}(pointer(buf)), dbuf, bytes, 2)
      for r in 0:st.np-1
        r == root || put!(st.boxes[r + 1], (st.rank, buf))
      end
    else
      buf = mailbox_recv(st, root)
      length(buf) == bytes || error("broadcast of $bytes bytes received $(length(buf))")
      GC.@preserve buf hip_copy(dbuf, Ptr{Cvoid}(pointer(buf)), bytes, 1)
    end
    return Int32(0)
  catch err
    @error "dhqr broadcast callback failed" exception = err
    return Int32(1)
  end
end

function cb_allreduce(user::Ptr{Cvoid}, dbuf::Ptr{Cvoid}, count::Int64, stream::Ptr{Cvoid})::Int32   # in-place sum of Float64
  try
    st = _cb[]::CallbackState
    bytes = 8 * count
    buf = Vector{UInt8}(undef, bytes)
    GC.@preserve buf hip_copy(Ptr{Cvoid}(pointer(buf)), dbuf, bytes, 2)
    if st.rank == 0                       # rank 0 sums in rank order (deterministic), everybody receives the total
      acc = copy(reinterpret(Float64, buf))
      for r in 1:st.np-1
        acc .+= reinterpret(Float64, mailbox_recv(st, r))
      end
      buf = Vector{UInt8}(reinterpret(UInt8, acc))
      for r in 1:st.np-1
        put!(st.boxes[r + 1], (0, buf))
      end
    else
      put!(st.boxes[1], (st.rank, buf))
      buf = mailbox_recv(st, 0)
    end
    GC.@preserve buf hip_copy(dbuf, Ptr{Cvoid}(pointer(buf)), bytes, 1)
    return Int32(0)
  catch err
    @error "dhqr all-reduce callback failed" exception = err
    return Int32(1)
  end
end

"collective over the workers: bind this worker (rank `rank` of `nranks`, 0-based) to GPU `device` with Julia carrying the
collectives (workers that share a GPU); `boxes[i]` is the mailbox of rank i-1"
function comm_init_callbacks(boxes, nranks::Integer, rank::Integer, device::Integer, key=nothing)
  first_time = _comm_key[] === nothing && _comm[] == C_NULL
  comm_free()
  _cb[] = CallbackState(collect(boxes), Int(nranks), Int(rank), [Vector{Vector{UInt8}}() for _ in 1:nranks])
  bc = @cfunction(cb_bcast, Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}))
  ar = @cfunction(cb_allreduce, Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}))
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:dhqr_comm_create_callbacks, libdhqr), Int32,
              (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
              h, context(device), Int32(nranks), Int32(rank), bc, ar, C_NULL))
  _comm[] = h[]
  _comm_key[] = key
  first_time && atexit(comm_free)
  return nothing
end

"collective bootstrap over the workers `ws` (once per (workers, devices), not per call): returns the key"
function ensure_comm(ws, devices)
  np = length(ws)
  devs = if devices === nothing            # `\\` after qr!(A; devices=...): reuse what qr! bound the workers to
    cached = remotecall_fetch(comm_devices, ws[1], ws)
    cached === nothing ? default_devices(ws) : cached
  else
    collect(devices)
  end
  key = (ws, devs)
  if !all(remotecall_fetch(comm_cached, p, key) for p in ws)
    if allunique(devs)                                                   # one GPU per worker: RCCL over xGMI
      id = remotecall_fetch(comm_unique_id, ws[1])                       # replaces the SharedArray bootstrap (src:301-304)
      @sync for (i, p) in enumerate(ws)                                  # ncclCommInitRank is collective
        @async remotecall_wait(comm_init, p, id, np, i - 1, devs[i], key)
      end
    else                                                                 # workers share a GPU: collectives through Julia
      boxes = [remotecall_fetch(mailbox_create, p) for p in ws]
      @sync for (i, p) in enumerate(ws)
        @async remotecall_wait(comm_init_callbacks, p, boxes, np, i - 1, devs[i], key)
      end
    end
  end
  return key
end

"number of HIP devices this process sees"
function device_count()
  c = Ref{Int32}(0)
  check(ccall((:dhqr_device_count, libdhqr), Int32, (Ref{Int32},), c))
  return Int(c[])
end

"the columns DistributedArrays' default split gives worker `rank` (0-based) of `np` -- what dhqr_cs_qr_darray_* assumes"
function contiguous_range(n::Integer, np::Integer, rank::Integer)
  lo = Ref{Int64}(0); hi = Ref{Int64}(0)
  ccall((:dhqr_cs_contiguous_range, libdhqr), Cvoid, (Int64, Int32, Int32, Ref{Int64}, Ref{Int64}),
        Int64(n), Int32(np), Int32(rank), lo, hi)
  return (Int(lo[]) + 1):Int(hi[])            # 0-based half-open -> 1-based inclusive
end

"a worker's column block must be full-height (src:33) and the default contiguous split (test/runtests.jl:71)"
function check_layout(A::DArray, rank::Integer, np::Integer)
  rows, cols = DistributedArrays.localindices(A)
  rows == 1:size(A, 1) || throw(ArgumentError("every worker must own full rows (src:33)"))
  cols == contiguous_range(size(A, 2), np, rank) ||
    throw(ArgumentError("column block $cols of worker $(myid()) is not DistributedArrays' default split"))
  return nothing
end

# executed ON a worker: its part of householder!(A::DArray, α) / of qrA \ b.  A DArray travels as a reference: on a
# worker that holds a chunk, localpart(A) is that worker's own storage, factored in place like src:122-148 does.
function householder_worker!(A::DArray{T, 2}, rank::Integer, np::Integer) where {T<:Union{Float64, ComplexF64}}
  check_layout(A, rank, np)
  m, n = size(A)
  al = zeros(T, n)
  householder_local!(localpart(A), m, n, al)
  return al
end
function solve_worker(A::DArray{T, 2}, rank::Integer, np::Integer, α::Vector{T}, b::Vector{T}) where {T<:Union{Float64, ComplexF64}}
  check_layout(A, rank, np)
  m, n = size(A)
  return solve_local(localpart(A), m, n, α, b)
end

# householder!(A::DArray, α) -- src:115-120.  ONE collective call per worker (the reference visits the owners in turn
# and sends every column to every process, src:138-143).  α may be the SharedArray of src:301-304 or a plain Vector.
function householder!(A::DArray{T, 2}, α::AbstractVector{T}; devices=nothing) where {T<:Union{Float64, ComplexF64}}
  ws = vec(procs(A))
  np = length(ws)
  ensure_comm(ws, devices)
  futs = [remotecall(householder_worker!, p, A, i - 1, np) for (i, p) in enumerate(ws)]
  als = map(fetch, futs)                       # fetch rethrows a worker's exception
  α .= als[1]                                  # the library returns α replicated; the master fills the shared vector
  return (A, α)
end

function qr!(A::DArray{T, 2}; devices=nothing) where {T<:Union{Float64, ComplexF64}}   # src:311-315
  H = DistributedHouseholderQRStruct(A)        # α::SharedArray, src:301-304
  householder!(H.A, H.α; devices=devices)
  return H
end

# solve_householder!(b, H::DArray, α) -- src:284-294 with the distributed phases src:226-230 (Q'b, owners in turn) and
# src:256-270 (back substitution, partial dots summed over the owners): ONE collective call per worker on its factored
# block; b[1:n] is overwritten with x like the reference leaves it, x is returned.  b may be the SharedArray of src:318.
function solve_householder!(b::AbstractVector{T}, A::DArray{T, 2}, α::AbstractVector{T}; devices=nothing) where {T<:Union{Float64, ComplexF64}}
  ws = vec(procs(A))
  np = length(ws)
  m, n = size(A)
  length(b) == m || throw(DimensionMismatch("b has length $(length(b)), the matrix $m rows"))
  ensure_comm(ws, devices)
  αv = Vector{T}(α); bv = Vector{T}(b)         # plain copies travel to the workers
  futs = [remotecall(solve_worker, p, A, i - 1, np, αv, bv) for (i, p) in enumerate(ws)]
  xs = map(fetch, futs)
  x = xs[1]                                    # x is replicated
  b[1:n] .= x
  return x
end

# qrA \ b for qrA = qr!(A::DArray) -- src:317-321; what test/runtests.jl:77-78 calls
function LinearAlgebra.:(\)(H::DistributedHouseholderQRStruct{<:DArray}, b::AbstractVector)
  s = SharedArray(Vector{eltype(H.A)}(b))      # src:318
  return solve_householder!(s, H.A, H.α)
end

alphafactor(x::Real) = -sign(x)   # src:8 (kept for API completeness; the device applies the same rule)
alphafactor(x::Complex) = -exp(im * angle(x))   # src:9

end # module
