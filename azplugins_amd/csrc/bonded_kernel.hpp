// bonded_kernel.hpp -- the outer kernel and the launcher of every bonded-group force: bonds (bond_forces.hip), angles
// (angle_forces.hip) and dihedrals (dihedral_forces.hip).
//
// bonded_forces_kernel<G, E> knows no geometry and no potential. One lane per local particle, no atomics: the lane
// walks its table entries in order and keeps, of each group, the force on its own position and its share of the
// energy and of the virial, so two calls give the same bits whatever the block size. Table columns are particle-major
// (entry s of particle i at s * pitch + i): every table read is coalesced; the partner positions are the only gathers.
// The per-type parameters are staged in LDS.
//
// A geometry policy G holds what differs between the kinds:
//   Args              its public argument struct of include/azp.h
//   Entry             one table entry as the kernel keeps it
//   Own               what the lane holds of its own row of pos (double3, or double4 to keep w)
//   PARTNERS          the other members of a group (1, 2, 3): partner rows gathered per entry
//   BATCH             the leading table columns that are loaded together (see below)
//   FLAGS             whether an evaluator can reject its parameters and raise the device flag word
//   tables(args, k)   host: the table pointers, the counts and the number of types out of Args; false if one is missing
//   block_size_ok(bs) host: the block sizes the kind accepts
//   own(pos, idx), unused(idx), load(a, at), partner(entry, k)
//   one<E>(a, s_params, p, entry, q, sums, d_flags)   the per-group body
// An evaluator E holds Params and eval(); what eval() takes is between it and its G.
//
// The first BATCH table columns of every lane are loaded together, then their PARTNERS * BATCH partner positions
// together: two dependent round trips for the batch instead of two per group. Entries past BATCH take the tail loop.
// Unused batch slots point at the lane's own (cached) row. BATCH is a register trade, chosen per kind.
#pragma once
#include "azp_device.hpp"
#include "pair_kernel_host.hpp"

namespace azp
{
struct BondedKArgs
    {
    double* force;
    double* virial;
    uint64_t virial_pitch;
    const double* pos;
    const void* table;      // G::Entry words, particle-major
    const uint32_t* table2; // bonds only: HOOMD keeps the position in the bond in a column of its own (bond_pos)
    const uint32_t* counts;
    uint64_t pitch;
    BoxDev box;
    uint32_t N;
    uint32_t n_types;
    uint32_t compute_virial;
    uint32_t _pad;
    };

// what one lane accumulates: force, energy share, the six virial rows
struct BondedSums
    {
    double fx, fy, fz, pe;
    double v[6];
    };

template<class G, class E>
__global__ void __launch_bounds__(256) bonded_forces_kernel(const BondedKArgs a, const typename E::Params* __restrict__ params,
                                                            unsigned int* __restrict__ d_flags)
    {
    typedef typename E::Params Params;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Params* s_params = reinterpret_cast<Params*>(s_raw);
    for (uint32_t t = threadIdx.x; t < a.n_types; t += blockDim.x)
        s_params[t] = params[t];
    __syncthreads();

    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const uint32_t n = a.counts[idx];
    const typename G::Own p = G::own(a.pos, idx);
    BondedSums sums = {0.0, 0.0, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
    constexpr uint32_t BATCH = G::BATCH, PARTNERS = G::PARTNERS;
    typename G::Entry ent[BATCH];
#pragma unroll
    for (uint32_t b = 0; b < BATCH; ++b)
        {
        ent[b] = G::unused(idx);
        if (b < n)
            ent[b] = G::load(a, (uint64_t)b * a.pitch + idx);
        }
    double3 q[BATCH][PARTNERS];
#pragma unroll
    for (uint32_t b = 0; b < BATCH; ++b)
#pragma unroll
        for (uint32_t k = 0; k < PARTNERS; ++k)
            q[b][k] = load_scalar3_of4(a.pos, G::partner(ent[b], k));
#pragma unroll
    for (uint32_t b = 0; b < BATCH; ++b)
        if (b < n)
            G::template one<E>(a, s_params, p, ent[b], q[b], sums, d_flags);
    for (uint32_t b = BATCH; b < n; ++b)
        {
        const typename G::Entry e = G::load(a, (uint64_t)b * a.pitch + idx);
        double3 qe[PARTNERS];
#pragma unroll
        for (uint32_t k = 0; k < PARTNERS; ++k)
            qe[k] = load_scalar3_of4(a.pos, G::partner(e, k));
        G::template one<E>(a, s_params, p, e, qe, sums, d_flags);
        }
    store_scalar4(a.force, idx, sums.fx, sums.fy, sums.fz, sums.pe);
    if (a.compute_virial)
        {
#pragma unroll
        for (int c = 0; c < 6; ++c)
            a.virial[(uint64_t)c * a.virial_pitch + idx] = sums.v[c];
        }
    }

// d_flags is looked at (and required) only where G::FLAGS is set. N == 0 succeeds before any array is looked at.
template<class G, class E>
static int launch_bonded(const typename G::Args* args, const typename E::Params* d_params, unsigned int* d_flags, void* stream)
    {
    if (!args || (G::FLAGS && (!d_params || !d_flags)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    BondedKArgs k;
    k.table2 = nullptr;
    if (!G::tables(*args, k) || !d_params || !args->d_force || !args->d_pos || args->pitch < args->N || k.n_types == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->compute_virial && (!args->d_virial || args->virial_pitch < args->N))
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    if (!G::block_size_ok(bs))
        return AZP_ERROR_INVALID_ARGUMENT;
    const size_t lds = sizeof(typename E::Params) * (size_t)k.n_types;
    if (lds > 64 * 1024)
        return AZP_ERROR_TOO_MANY_TYPES;
    k.force = args->d_force;
    k.virial = args->d_virial;
    k.virial_pitch = args->virial_pitch;
    k.pos = args->d_pos;
    k.pitch = args->pitch;
    k.box = make_box_dev(args->box);
    k.N = args->N;
    k.compute_virial = args->compute_virial;
    k._pad = 0;
    const uint32_t grid = (args->N + bs - 1) / bs;
    LaunchInfo& li = last_launch();
    li.block_size = bs; li.tpp = 1; li.grid = grid; li.lds_bytes = (uint32_t)lds;
    hipLaunchKernelGGL((bonded_forces_kernel<G, E>), dim3(grid), dim3(bs), lds, static_cast<hipStream_t>(stream), k, d_params,
                       d_flags);
    return (int)hipGetLastError();
    }
} // namespace azp
