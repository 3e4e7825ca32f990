# DwaveHMCGPU.jl — Julia `ccall` binding of libdwhmc.so (include/dwhmc.h).
#
# Drop-in for the hot path of DwaveHMC.jl: `GPUCache` replaces `ComputeCache`
# and the methods below extend init_static_H!/update_H_BdG!/diagonalize_H_BdG!/
# compute_forces!/compute_total_energy/hmc_sweep!/measure_observables/
# measure_transport_and_spectra for it, with the reference's argument order and
# mutation semantics (src/Hamiltonian.jl, src/Observables.jl, src/HMC.jl) —
# every call `run_simulation` (src/Simulation.jl:84-171) makes on its cache.
# `DwaveHMCGPU.run_simulation` is the reference's own driver, evaluated from
# its source with the one cache-constructing call swapped (see the end of
# this file).  Not executable in this image (no Julia, SURVEY.md F4); the ABI
# it binds is exercised through ctypes by tests/ (tests/test_gpu_parity.py,
# tests/test_gpu_assembly.py, tests/test_simulation.py).
module DwaveHMCGPU

using DwaveHMC
using Random
using Dates, Printf, DelimitedFiles, JLD2          # what src/Simulation.jl:1-4 uses
import DwaveHMC: init_static_H!, update_H_BdG!, diagonalize_H_BdG!, compute_forces!,
                 compute_total_energy, hmc_sweep!, measure_observables,
                 measure_transport_and_spectra

const libdwhmc = get(ENV, "DWHMC_LIB", joinpath(@__DIR__, "..", "hybrid-monte-carlo-for-d-wave-sc_amd", "libdwhmc.so"))

struct DwhError <: Exception
    code::Cint
    msg::String
end

function check(ctx::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:dwh_last_error, libdwhmc), Cstring, (Ptr{Cvoid},), ctx))
    rc == -1 && throw(ArgumentError(msg))
    throw(DwhError(rc, msg))
end

"""GPU-resident replacement of ComputeCache (src/Types.jl:145-212)."""
mutable struct GPUCache
    ctx::Ptr{Cvoid}
    forces::Matrix{ComplexF64}
    E_fermion::Float64
    device::Int32
    delta_cap::Float64
end

function GPUCache(p::ModelParameters; device::Integer=0, delta_cap::Real=0.0)   # <= 0: the ABI default (include/dwhmc.h)
    c = GPUCache(C_NULL, zeros(ComplexF64, p.N, 2), 0.0, Int32(device), Float64(delta_cap))
    finalizer(c) do c
        c.ctx == C_NULL || ccall((:dwh_destroy, libdwhmc), Cvoid, (Ptr{Cvoid},), c.ctx)
        c.ctx = C_NULL
    end
    return c
end

# src/Hamiltonian.jl:10-47 — the disorder is consumed here, as in the reference
function init_static_H!(cache::GPUCache, p::ModelParameters, state::SimulationState)
    cache.ctx == C_NULL || ccall((:dwh_destroy, libdwhmc), Cvoid, (Ptr{Cvoid},), cache.ctx)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve p state begin
        rc = ccall((:dwh_create_batched, libdwhmc), Cint,
                   (Ref{Ptr{Cvoid}}, Int64, Int64, Float64, Float64, Float64, Float64, Float64,
                    Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}, Float64, Int32),
                   ref, p.Lx, p.Ly, p.t, p.tp, p.μ, p.β, p.J, p.nn_table, p.nnn_table,
                   1, state.disorder_pot, cache.delta_cap, cache.device)
    end
    check(C_NULL, rc)
    cache.ctx = ref[]
    return nothing
end

# src/Hamiltonian.jl:55-86 — Δ is Julia's column-major N×2 ComplexF64 = the ABI layout
function update_H_BdG!(cache::GPUCache, p::ModelParameters, state::SimulationState)
    GC.@preserve state check(cache.ctx, ccall((:dwh_update_pairing, libdwhmc), Cint,
                                              (Ptr{Cvoid}, Ptr{ComplexF64}), cache.ctx, state.Δ))
end

# src/Hamiltonian.jl:96-114 replacement (pole-expanded no-pivot LU, no eigenpairs)
function diagonalize_H_BdG!(cache::GPUCache, p::ModelParameters)
    check(cache.ctx, ccall((:dwh_factorize, libdwhmc), Cint, (Ptr{Cvoid},), cache.ctx))
    ef = Ref{Float64}(0.0)
    check(cache.ctx, ccall((:dwh_fermion_energy, libdwhmc), Cint, (Ptr{Cvoid}, Ref{Float64}), cache.ctx, ef))
    cache.E_fermion = ef[]
    return nothing
end

# src/Observables.jl:14-62
function compute_forces!(cache::GPUCache, p::ModelParameters, state::SimulationState)
    GC.@preserve state cache check(cache.ctx, ccall((:dwh_forces, libdwhmc), Cint,
                                                    (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                                                    cache.ctx, state.Δ, cache.forces))
end

# src/HMC.jl:12-41
function compute_total_energy(cache::GPUCache, p::ModelParameters, state::SimulationState)
    GC.@preserve state check(cache.ctx, ccall((:dwh_set_state, libdwhmc), Cint,
                                              (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                                              cache.ctx, state.Δ, state.π))
    h = Ref{Float64}(0.0)
    check(cache.ctx, ccall((:dwh_total_energy, libdwhmc), Cint, (Ptr{Cvoid}, Float64, Ref{Float64}),
                           cache.ctx, p.mass, h))
    return h[]
end

# src/HMC.jl:71-144.  The reference's own RNG draws are taken here in the
# reference's order: randn! for the momenta (:53) before the trajectory, and
# rand() only when ΔH >= 0 (the short-circuit `ΔH < 0 || rand() < exp(-ΔH)`
# of :128), so a seeded Julia RNG is consumed exactly as DwaveHMC consumes it.
# The device runs the trajectory (dwh_hmc_trajectory) and, after the host's
# decision, restores a rejected chain (dwh_hmc_finish).
function hmc_sweep!(cache::GPUCache, p::ModelParameters, state::SimulationState; Nt::Int, dt::Float64)
    noise = randn(ComplexF64, p.N, 2)
    dH = Ref{Float64}(0.0)
    GC.@preserve state noise begin
        check(cache.ctx, ccall((:dwh_set_state, libdwhmc), Cint,
                               (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}), cache.ctx, state.Δ, C_NULL))
        check(cache.ctx, ccall((:dwh_hmc_trajectory, libdwhmc), Cint,
                               (Ptr{Cvoid}, Ptr{ComplexF64}, Int64, Float64, Float64, Ref{Float64}),
                               cache.ctx, noise, Nt, dt, p.mass, dH))
        ΔH = dH[]
        accepted = ΔH < 0 || rand() < exp(-ΔH)
        check(cache.ctx, ccall((:dwh_hmc_finish, libdwhmc), Cint, (Ptr{Cvoid}, Ref{UInt8}),
                               cache.ctx, Ref{UInt8}(accepted ? 1 : 0)))
        check(cache.ctx, ccall((:dwh_get_state, libdwhmc), Cint,
                               (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}), cache.ctx, state.Δ, state.π))
    end
    ef = Ref{Float64}(0.0)
    check(cache.ctx, ccall((:dwh_fermion_energy, libdwhmc), Cint, (Ptr{Cvoid}, Ref{Float64}), cache.ctx, ef))
    cache.E_fermion = ef[]
    return accepted, ΔH
end

# The integrator of every later hmc_sweep! on this cache (dwh_set_integrator,
# include/dwhmc.h): :leapfrog (the reference's, src/HMC.jl:88-118, and the
# default without this call), :omelyan2 (two factorisations per step; λ its
# parameter, default the minimum-norm value) or :custom with kick = a_0..a_S
# and drift = b_1..b_S.  Nt of hmc_sweep! stays the number of steps.  Call it
# after init_static_H! (which creates the context).  Like the rest of this
# file it has not been run (no Julia in this image); the entry it binds is
# exercised through ctypes by tests/test_integrator_gpu.py.
const OMELYAN2_LAMBDA = 0.1931833275037836
function set_integrator!(cache::GPUCache, kind::Symbol=:omelyan2; λ::Float64=OMELYAN2_LAMBDA,
                         kick::Vector{Float64}=Float64[], drift::Vector{Float64}=Float64[])
    code = kind === :leapfrog ? Int32(0) : kind === :omelyan2 ? Int32(1) : kind === :custom ? Int32(2) :
           throw(ArgumentError("integrator kind must be :leapfrog, :omelyan2 or :custom"))
    kind === :custom && length(kick) != length(drift) + 1 &&
        throw(ArgumentError("custom integrator: kick has one entry more than drift"))
    GC.@preserve kick drift check(cache.ctx, ccall((:dwh_set_integrator, libdwhmc), Cint,
                                                   (Ptr{Cvoid}, Int32, Float64, Int64, Ptr{Float64}, Ptr{Float64}),
                                                   cache.ctx, code, λ, length(drift),
                                                   kind === :custom ? pointer(kick) : C_NULL,
                                                   kind === :custom ? pointer(drift) : C_NULL))
    return nothing
end

# n sweeps on the throughput path with the device's sweep log (dwh_load_draws,
# dwh_sweep_log, dwh_run_sweeps and the log's readers, include/dwhmc.h): the
# draws of all sweeps are taken first — per sweep randn(ComplexF64, N, 2), then
# one rand(), always, since the device wants every uniform before its first
# sweep (the reference's "rand() only when ΔH >= 0", src/HMC.jl:128, cannot be
# kept) — and per sweep the device records the observables (the nine fields of
# ObservablesResult, then E_f, Tr ρ_hh, Σ|Δ|²), with field_sq the structure
# factors S_d(q), S_s(q) of the pairing field, and with snap_every > 0 the Δ
# after the sweeps snap_offset, snap_offset + snap_every, ... (0-based within
# the call).  Returns (accepted, ΔH, obs 12 x n, sq Lx x Ly x 2 x n or nothing,
# snapshot sweeps, Δ snapshots N x 2 x m); state.Δ, state.π and the cache end
# at the last sweep.  Not run, like the rest of this file; the entries are
# exercised through ctypes by tests/test_sweep_log_gpu.py.
const DWH_LOG_OBS, DWH_LOG_FIELD_SQ, DWH_LOG_SNAPSHOT = Int32(1), Int32(2), Int32(4)
const DWH_OBS_FIELDS = 12
function run_sweeps_logged!(cache::GPUCache, p::ModelParameters, state::SimulationState, n::Int; Nt::Int,
                            dt::Float64, field_sq::Bool=false, snap_every::Int=0, snap_offset::Int=0)
    noise = zeros(ComplexF64, p.N, 2, n)
    uniform = zeros(n)
    for k in 1:n
        noise[:, :, k] = randn(ComplexF64, p.N, 2)
        uniform[k] = rand()
    end
    what = DWH_LOG_OBS | (field_sq ? DWH_LOG_FIELD_SQ : Int32(0)) | (snap_every > 0 ? DWH_LOG_SNAPSHOT : Int32(0))
    accepted, dH = zeros(UInt8, n), zeros(n)
    obs = zeros(DWH_OBS_FIELDS, n)
    sq = field_sq ? zeros(p.Lx, p.Ly, 2, n) : nothing
    nsnap = Ref{Int64}(0)
    GC.@preserve state noise uniform accepted dH obs begin
        check(cache.ctx, ccall((:dwh_set_state, libdwhmc), Cint,
                               (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}), cache.ctx, state.Δ, C_NULL))
        check(cache.ctx, ccall((:dwh_load_draws, libdwhmc), Cint, (Ptr{Cvoid}, Int64, Ptr{ComplexF64}, Ptr{Float64}),
                               cache.ctx, n, noise, uniform))
        check(cache.ctx, ccall((:dwh_sweep_log, libdwhmc), Cint, (Ptr{Cvoid}, Int32, Int64, Int64),
                               cache.ctx, what, snap_every, snap_offset))
        check(cache.ctx, ccall((:dwh_run_sweeps, libdwhmc), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Float64, Float64),
                               cache.ctx, 0, n, Nt, dt, p.mass))
        check(cache.ctx, ccall((:dwh_sweep_results, libdwhmc), Cint,
                               (Ptr{Cvoid}, Int64, Int64, Ptr{UInt8}, Ptr{Float64}), cache.ctx, 0, n, accepted, dH))
        check(cache.ctx, ccall((:dwh_sweep_observables, libdwhmc), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}),
                               cache.ctx, 0, n, obs))
        if field_sq
            GC.@preserve sq check(cache.ctx, ccall((:dwh_sweep_field_sq, libdwhmc), Cint,
                                                   (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}), cache.ctx, 0, n, sq))
        end
    end
    sweeps, snaps = Int64[], zeros(ComplexF64, p.N, 2, 0)
    if snap_every > 0
        check(cache.ctx, ccall((:dwh_sweep_snapshots, libdwhmc), Cint,
                               (Ptr{Cvoid}, Int64, Int64, Ref{Int64}, Ptr{Int64}, Ptr{ComplexF64}),
                               cache.ctx, 0, n, nsnap, C_NULL, C_NULL))
        sweeps, snaps = zeros(Int64, nsnap[]), zeros(ComplexF64, p.N, 2, nsnap[])
        GC.@preserve sweeps snaps check(cache.ctx, ccall((:dwh_sweep_snapshots, libdwhmc), Cint,
                                                         (Ptr{Cvoid}, Int64, Int64, Ref{Int64}, Ptr{Int64},
                                                          Ptr{ComplexF64}), cache.ctx, 0, n, nsnap, sweeps, snaps))
    end
    GC.@preserve state check(cache.ctx, ccall((:dwh_get_state, libdwhmc), Cint,
                                              (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{ComplexF64}), cache.ctx, state.Δ,
                                              state.π))
    n > 0 && (cache.E_fermion = obs[10, n])
    return accepted .!= 0, dH, obs, sq, sweeps, snaps
end

# src/Observables.jl:88-222 from what the factorisation caches instead of the
# eigenpairs: E_f (dwh_fermion_energy, = -Σ_{E>0}(βE + 2 log1pexp(-βE)) of
# :147-156), P_ij (dwh_pairing, the ρ sums of :172-198) and Tr ρ_hh
# (dwh_hole_trace; hole_conc = 2 Tr ρ_hh / N - 1, SURVEY.md I4, = the u/v
# tanh sum of :120-145).  Same arithmetic as the reference on Δ, same fields.
function measure_observables(cache::GPUCache, p::ModelParameters, state::SimulationState)
    N = p.N
    sum_amp = 0.0
    sum_local = 0.0
    sum_global = 0.0 + 0.0im
    @inbounds for i in 1:N
        dx = state.Δ[i, 1]
        dy = state.Δ[i, 2]
        sum_amp += 0.5 * (abs(dx) + abs(dy))
        sum_local += 0.5 * abs(dx - dy)
        sum_global += 0.5 * (dx - dy)
    end
    ef = Ref{Float64}(0.0)
    trhh = Ref{Float64}(0.0)
    P = zeros(ComplexF64, N, 2)
    check(cache.ctx, ccall((:dwh_fermion_energy, libdwhmc), Cint, (Ptr{Cvoid}, Ref{Float64}), cache.ctx, ef))
    check(cache.ctx, ccall((:dwh_hole_trace, libdwhmc), Cint, (Ptr{Cvoid}, Ref{Float64}), cache.ctx, trhh))
    GC.@preserve P check(cache.ctx, ccall((:dwh_pairing, libdwhmc), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}),
                                          cache.ctx, P))
    E_boson = p.β / (2 * p.J) * sum(abs2, state.Δ)
    sum_diff = 0.0
    sum_pair_global = 0.0 + 0.0im
    sum_pair_local = 0.0
    @inbounds for i in 1:N
        P_x, P_y = P[i, 1], P[i, 2]
        sum_diff += (abs(state.Δ[i, 1] - p.J * P_x) + abs(state.Δ[i, 2] - p.J * P_y)) / 2.0
        term = p.J * 0.5 * (P_x - P_y)
        sum_pair_local += abs(term)
        sum_pair_global += term
    end
    return DwaveHMC.ObservablesResult((ef[] + E_boson) / N, sum_amp / N, sum_local / N,
                                      abs(sum_global / N), abs2(sum_global / N), 2.0 * trhh[] / N - 1.0,
                                      sum_diff / N, abs(sum_pair_global / N), sum_pair_local / N)
end

# src/Observables.jl:314-526 on the device (eigenpairs by the library's own
# Hermitian eigensolver, sums in HIP kernels) for the Δ the context holds; same SpectrumResult.
function measure_transport_and_spectra(cache::GPUCache, p::ModelParameters)
    nw, nd = Ref{Int64}(0), Ref{Int64}(0)
    check(C_NULL, ccall((:dwh_transport_grid, libdwhmc), Cint,
                        (Float64, Float64, Float64, Ref{Int64}, Ref{Int64}), p.η, p.Δω, p.ω_max, nw, nd))
    st, dc = Ref{Float64}(0.0), Ref{Float64}(0.0)
    σ, dos, dos_AN = zeros(nw[]), zeros(nd[]), zeros(nd[])
    ak = zeros(p.Lx, p.Ly)
    check(cache.ctx, ccall((:dwh_measure_transport, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Float64, Float64, Float64, Ref{Float64}, Ref{Float64},
                            Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
                           cache.ctx, 0, p.η, p.Δω, p.ω_max, st, dc, σ, nw[], dos, dos_AN, nd[], ak))
    return DwaveHMC.SpectrumResult(st[], dc[], collect(p.ω_min:p.Δω:p.ω_max), σ,
                                   collect(-p.ω_max:p.Δω:p.ω_max), dos, dos_AN, ak)
end

# The resolved spectra SpectrumResult leaves out (src/Observables.jl:305-307), for
# the Δ the context holds, on the window first + q·stride (q < count, 0-based
# points) of the DOS grid -ω_max:Δω:ω_max; count = nothing: to the end of the grid.
#   ldos[x, y, q] = Σ_n |u_n(i)|² L(ω_q - E_n),         i = x + Lx·y
#   akw[kx, ky, q] = (1/N) Σ_n |û_n(k)|² L(ω_q - E_n)   (FFTW's forward sign)
# Returns (ω, ldos, akw); a map switched off comes back as `nothing`.
function measure_spectral_maps(cache::GPUCache, p::ModelParameters; first::Integer=0,
                               count::Union{Nothing,Integer}=nothing, stride::Integer=1,
                               ldos::Bool=true, akw::Bool=true)
    if count === nothing
        nw, nd = Ref{Int64}(0), Ref{Int64}(0)
        check(C_NULL, ccall((:dwh_transport_grid, libdwhmc), Cint,
                            (Float64, Float64, Float64, Ref{Int64}, Ref{Int64}), p.η, p.Δω, p.ω_max, nw, nd))
        count = (0 <= first < nd[] && stride >= 1) ? (nd[] - 1 - first) ÷ stride + 1 : 0
    end
    ω = zeros(max(count, 0))
    check(C_NULL, ccall((:dwh_spectral_window, libdwhmc), Cint,
                        (Float64, Float64, Float64, Int64, Int64, Int64, Ptr{Float64}),
                        p.η, p.Δω, p.ω_max, first, count, stride, ω))
    L = ldos ? zeros(p.Lx, p.Ly, count) : nothing
    A = akw ? zeros(p.Lx, p.Ly, count) : nothing
    GC.@preserve L A check(cache.ctx, ccall((:dwh_measure_spectral_maps, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{ComplexF64}, Float64, Float64, Float64,
                            Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                           cache.ctx, 0, 1, C_NULL, p.η, p.Δω, p.ω_max, first, count, stride,
                           L === nothing ? C_NULL : pointer(L), A === nothing ? C_NULL : pointer(A)))
    return ω, L, A
end

# The stiffness terms of src/Observables.jl:340-387 away from q = 0, for the Δ
# the context holds: Λ_αα(q, iΩ_l) of direction α (:x or :y) at the lattice
# momenta q = 2π (mx/Lx, my/Ly) of `q` (a vector of (mx, my), not reduced
# modulo L) and Ω_l = 2π l/β, l < n_matsubara, and the diamagnetic term of α.
# Returns (dia, Λ) with Λ[l + 1, k] for momentum q[k]; dia - Λ[1, k] at
# q = (0, 1), α = :x is the transverse (superfluid) limit.
function measure_current_response(cache::GPUCache, p::ModelParameters; direction::Symbol=:x,
                                  q::AbstractVector=[(0, 1)], n_matsubara::Integer=1)
    direction in (:x, :y) || throw(ArgumentError("direction must be :x or :y"))
    nq = length(q)
    qa = Matrix{Int64}(undef, 2, nq)
    for (k, (mx, my)) in enumerate(q)
        qa[1, k], qa[2, k] = mx, my
    end
    dia = Ref{Float64}(0.0)
    Λ = zeros(max(n_matsubara, 0), nq)
    GC.@preserve qa Λ check(cache.ctx, ccall((:dwh_measure_current_response, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{ComplexF64}, Int32, Int64, Ptr{Int64}, Int64,
                            Ref{Float64}, Ptr{Float64}),
                           cache.ctx, 0, 1, C_NULL, direction === :x ? 0 : 1, nq, pointer(qa), n_matsubara,
                           dia, pointer(Λ)))
    return dia[], Λ
end

# The response of any one-body operators O_k = Σ_ij V_ij (c†_{i↑} c_{j↑} + s_k
# c†_{i↓} c_{j↓}) for the Δ the context holds (dwh_measure_operator_response;
# Nambu matrix V ⊕ (-s Vᵀ)), the generic CSR form: one pattern for all
# operators, 0-based (`rowptr` of N + 1 entries, `col` of nnz entries,
# duplicates add up), `val[e, k]` the nnz values of operator k, `spin_sign[k]`
# = ±1.  Returns (χ, χ2): χ[l + 1, k] at Ω_l = 2π l/β, l < n_matsubara, in the
# conventions of measure_current_response's Λ, and χ2[j + 1, k] = χ''(ω_j) on
# ω_j = ω_start + j·ω_step, j < n_ω (σ(ω)'s conventions without its 1/ω; ω of
# either sign; needs η > 0).  n_matsubara = 0 or n_ω = 0 skips that part.
function measure_operator_response(cache::GPUCache, p::ModelParameters, rowptr::Vector{Int64},
                                   col::Vector{Int64}, val::Matrix{ComplexF64}, spin_sign::Vector{Int32};
                                   n_matsubara::Integer=1, η::Real=p.η, ω_start::Real=0.0, ω_step::Real=0.0,
                                   n_ω::Integer=0)
    nnz, nops = size(val)
    length(col) == nnz || throw(ArgumentError("val must be nnz x nops with nnz = length(col)"))
    length(rowptr) == p.N + 1 || throw(ArgumentError("rowptr must have N + 1 entries"))
    length(spin_sign) == nops || throw(ArgumentError("one spin sign per operator"))
    χ = zeros(max(n_matsubara, 0), nops)
    χ2 = zeros(max(n_ω, 0), nops)
    GC.@preserve rowptr col val spin_sign χ χ2 check(cache.ctx, ccall((:dwh_measure_operator_response, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{ComplexF64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64,
                            Ptr{ComplexF64}, Ptr{Int32}, Int64, Ptr{Float64}, Float64, Float64, Float64, Int64,
                            Ptr{Float64}),
                           cache.ctx, 0, 1, C_NULL, nops, pointer(rowptr), pointer(col), nnz, pointer(val),
                           pointer(spin_sign), n_matsubara, n_matsubara > 0 ? pointer(χ) : C_NULL,
                           Float64(η), Float64(ω_start), Float64(ω_step), n_ω, n_ω > 0 ? pointer(χ2) : C_NULL))
    return χ, χ2
end

# The cross response <O_a ; O_b†> of general Nambu vertices O_k = Ψ† W_k Ψ,
# Ψ = (c_{i↑}; c†_{i↓}), pairing blocks included, for the Δ the context holds
# (dwh_measure_nambu_response), the CSR form: one pattern with 2N rows for all
# vertices, 0-based (`rowptr` of 2N + 1 entries, `col` of nnz entries in
# [0, 2N), duplicates add up), `val[e, k]` the nnz values of vertex k, and
# `pairs[:, p]` = (a_p, b_p), 0-based vertex indices.  Returns (χ, χ2), both
# complex: χ[l + 1, p] = (1/N) Σ (f_n - f_m)/(ΔE - iΩ_l) X^a_nm conj(X^b_nm)
# with the l = 0 rules of measure_current_response, χ2[j + 1, p] on
# ω_j = ω_start + j·ω_step, j < n_ω.  n_matsubara = 0 or n_ω = 0 skips that
# part.  Not run; the same ABI call is exercised through ctypes by
# tests/test_nambu_response.py.
function measure_nambu_response(cache::GPUCache, p::ModelParameters, rowptr::Vector{Int64},
                                col::Vector{Int64}, val::Matrix{ComplexF64}, pairs::Matrix{Int64};
                                n_matsubara::Integer=1, η::Real=p.η, ω_start::Real=0.0, ω_step::Real=0.0,
                                n_ω::Integer=0)
    nnz, nops = size(val)
    length(col) == nnz || throw(ArgumentError("val must be nnz x nops with nnz = length(col)"))
    length(rowptr) == 2 * p.N + 1 || throw(ArgumentError("rowptr must have 2N + 1 entries"))
    size(pairs, 1) == 2 || throw(ArgumentError("pairs must be 2 x npairs"))
    npairs = size(pairs, 2)
    χ = zeros(ComplexF64, max(n_matsubara, 0), npairs)
    χ2 = zeros(ComplexF64, max(n_ω, 0), npairs)
    GC.@preserve rowptr col val pairs χ χ2 check(cache.ctx, ccall((:dwh_measure_nambu_response, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{ComplexF64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64,
                            Ptr{ComplexF64}, Int64, Ptr{Int64}, Int64, Ptr{ComplexF64}, Float64, Float64, Float64,
                            Int64, Ptr{ComplexF64}),
                           cache.ctx, 0, 1, C_NULL, nops, pointer(rowptr), pointer(col), nnz, pointer(val),
                           npairs, pointer(pairs), n_matsubara, n_matsubara > 0 ? pointer(χ) : C_NULL,
                           Float64(η), Float64(ω_start), Float64(ω_step), n_ω, n_ω > 0 ? pointer(χ2) : C_NULL))
    return χ, χ2
end

# Response maps for the Δ the context holds (dwh_measure_response_map): the
# linear-response density matrix D(z)[W_k] = U (w(z) ∘ Uᴴ W_k U) Uᴴ of every
# source vertex (the CSR form of measure_nambu_response) and the equal-time
# ρ = U f Uᴴ, at the Nambu index pairs `pattern[:, e]` = (a_e, b_e), 0-based in
# [0, 2N), any order, duplicates allowed.  z runs over the n_matsubara
# Matsubara indices, then the real frequencies `ω` (w = (f_n - f_m)/(ΔE - ω -
# iη); needs η > 0).  Returns (ρ, D): ρ[e + 1] and D[e + 1, z + 1, k + 1], both
# complex, no 1/N applied; Σ_e conj(B_e) D_e = N·χ of measure_nambu_response
# for the pair (W_k, B).  `rho = false` skips ρ (returned empty), no frequency
# at all skips D.  Not run; the same ABI call is exercised through
# ctypes by tests/test_response_map.py.
function measure_response_map(cache::GPUCache, p::ModelParameters, rowptr::Vector{Int64},
                              col::Vector{Int64}, val::Matrix{ComplexF64}, pattern::Matrix{Int64};
                              n_matsubara::Integer=1, η::Real=p.η, ω::Vector{Float64}=Float64[],
                              rho::Bool=true)
    nnz, nops = size(val)
    length(col) == nnz || throw(ArgumentError("val must be nnz x nops with nnz = length(col)"))
    length(rowptr) == 2 * p.N + 1 || throw(ArgumentError("rowptr must have 2N + 1 entries"))
    size(pattern, 1) == 2 || throw(ArgumentError("pattern must be 2 x npat"))
    npat = size(pattern, 2)
    prow, pcol = pattern[1, :], pattern[2, :]
    n_ω = length(ω)
    nz = max(n_matsubara, 0) + n_ω
    ρ = zeros(ComplexF64, rho ? npat : 0)
    D = zeros(ComplexF64, npat, nz, nz > 0 ? nops : 0)
    GC.@preserve rowptr col val prow pcol ω ρ D check(cache.ctx, ccall((:dwh_measure_response_map, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{ComplexF64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64,
                            Ptr{ComplexF64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Float64, Int64, Ptr{Float64},
                            Ptr{ComplexF64}, Ptr{ComplexF64}),
                           cache.ctx, 0, 1, C_NULL, nops, pointer(rowptr), pointer(col), nnz, pointer(val),
                           npat, pointer(prow), pointer(pcol), n_matsubara, Float64(η), n_ω,
                           n_ω > 0 ? pointer(ω) : C_NULL, rho ? pointer(ρ) : C_NULL, nz > 0 ? pointer(D) : C_NULL))
    return ρ, D
end

# Equal-time correlations for the Δ the context holds (dwh_measure_correlations):
# local families O_A(i) = Σ_t a Ψ†_r Ψ_c as one term table — the terms of family
# k at site i are tptr[k N + i + 1] + 1 : tptr[k N + i + 2] of (trow, tcol, tval),
# tptr, trow, tcol 0-based as the ABI takes them — and `pairs` (2 x npairs,
# 0-based family indices).  Returns (mean, corr, local): mean[i + 1, k + 1] =
# <O_k(i)>, corr[r + 1, p + 1] = (1/N) Σ_j G_p(j ⊕ r, j) and local[r + 1, q + 1,
# p + 1] = G_p(ref_q ⊕ r, ref_q) with G_AB(i, j) = <O_A(i) O_B(j)†> -
# <O_A(i)><O_B(j)†>; `ref` (0-based sites) empty skips local.  Not run; the same
# ABI call is exercised through ctypes by tests/test_correlations.py.
function measure_correlations(cache::GPUCache, p::ModelParameters, tptr::Vector{Int64}, trow::Vector{Int64},
                              tcol::Vector{Int64}, tval::Vector{ComplexF64}, pairs::Matrix{Int64};
                              ref::Vector{Int64}=Int64[])
    (length(tptr) - 1) % p.N == 0 || throw(ArgumentError("tptr must have nfam N + 1 entries"))
    size(pairs, 1) == 2 || throw(ArgumentError("pairs must be 2 x npairs"))
    nfam, npairs, nref = (length(tptr) - 1) ÷ p.N, size(pairs, 2), length(ref)
    m = zeros(ComplexF64, p.N, nfam)
    c = zeros(ComplexF64, p.N, npairs)
    l = zeros(ComplexF64, p.N, nref, npairs)
    GC.@preserve tptr trow tcol tval pairs ref m c l check(cache.ctx, ccall((:dwh_measure_correlations, libdwhmc), Cint,
                           (Ptr{Cvoid}, Int64, Int64, Ptr{ComplexF64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                            Ptr{ComplexF64}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{ComplexF64},
                            Ptr{ComplexF64}, Ptr{ComplexF64}),
                           cache.ctx, 0, 1, C_NULL, nfam, pointer(tptr), pointer(trow), pointer(tcol), pointer(tval),
                           npairs, pointer(pairs), nref, nref > 0 ? pointer(ref) : C_NULL, pointer(m), pointer(c),
                           nref > 0 ? pointer(l) : C_NULL))
    return m, c, l
end

# ---------------------------------------------------------------------------
# run_simulation on the GPU.  The reference constructs its cache inside the
# driver (`cache = initialize_cache(p)`, src/Simulation.jl:82), so the driver
# is taken from DwaveHMC's own source file and evaluated here with exactly
# that call replaced by `GPUCache(p)`; every other line — adaptive Nt,
# observables.csv, transport.csv, JLD2 bins, log — is the reference's, and
# every cache-typed call in it (init_static_H!, update_H_BdG!,
# diagonalize_H_BdG! :84-86, hmc_sweep! :105/:153, measure_observables :157,
# measure_transport_and_spectra :171) dispatches to the methods above.
# ---------------------------------------------------------------------------
_swap_cache(x) = x
function _swap_cache(ex::Expr)
    if ex.head == :call && ex.args[1] === :initialize_cache
        return Expr(:call, :GPUCache, map(_swap_cache, ex.args[2:end])...)
    end
    return Expr(ex.head, map(_swap_cache, ex.args)...)
end

_defines(ex, name) = ex isa Expr && ((ex.head == :function && ex.args[1] isa Expr &&
                                      ex.args[1].args[1] === name) ||
                                     (ex.head == :macrocall && any(a -> _defines(a, name), ex.args)))

function __init__()
    src = read(joinpath(dirname(pathof(DwaveHMC)), "Simulation.jl"), String)
    top = Meta.parseall(src)
    n = 0
    for ex in top.args
        if _defines(ex, :run_simulation)
            Core.eval(@__MODULE__, _swap_cache(ex))
            n += 1
        end
    end
    n == 1 || error("DwaveHMCGPU: run_simulation not found in DwaveHMC's Simulation.jl")
end

end # module
