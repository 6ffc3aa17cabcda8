// The parent's forward and backward ladders, verbatim (gat_edge_kernels.hip of the commit before, lines 2196-2231 and 2242-2324), under other
// names: pick_fwd -> parent_pick_fwd, pick_bwd -> parent_pick_bwd.  They name the same, untouched kernel templates.  Included by pick_sweep.hip.
// Forward.  ext (EdgeFwdExtras were passed: masks and / or residual, bias, norm): the EXT instantiation of the kernel the default
// settings pick, one wave per block — the parity-tap form with alpha, else the group-per-row kernel where the shape has one, else the
// packed wave-per-row kernel.  The A/B switches of the default path (GAT_ROWGROUP, GAT_PACKED, GAT_CPL, GAT_FWD_WAVES) do not apply to
// it: only these instantiations exist.
// res (residual, bias or norm, always with ext): the fix-up kernel is the EXT form too — the masks alone leave it the plain one.
// pe (edge features, always with ext): the PE instantiation of the same kernel; the fix-up kernels never see the edge term.
template <int HD, int D, bool BF>
EdgePick parent_pick_fwd(const EdgeFwdArgs& a, bool ext, bool res, bool pe) {
    static_assert(D % 2 == 0, "every fast-path shape has an even D");
    constexpr int N3 = stash_n<HD, D>(), N2 = (HD >= 32 && D % 4 == 0) ? 4 : 2;
    constexpr int G3 = N3 != 0 ? 64 / (HD / (N3 != 0 ? N3 : 1)) : 1;             // rows per wave of the group-per-row kernel
    if (a.alpha != nullptr) {                                                     // parity-tap form: alpha (and scores) materialised
        const void* fix = res ? GAT_K(edge_fwd_fix_kernel<HD, D, true, true>) : GAT_K(edge_fwd_fix_kernel<HD, D, true>);
        if (pe) return {GAT_K(edge_fwd_kernel<HD, D, true, BF, true, true>), 256, 4, fix};
        return {ext ? GAT_K(edge_fwd_kernel<HD, D, true, BF, true>) : GAT_K(edge_fwd_kernel<HD, D, true, BF>), 256, 4, fix};
    }
    const void* fix = res ? GAT_K(edge_fwd_fix_kernel<HD, D, false, true>) : GAT_K(edge_fwd_fix_kernel<HD, D, false>);
    if (pe) {
        if constexpr (N3 != 0) return {GAT_K(edge_fwd3_kernel<HD, D, N3, BF, true, true>), 64, G3, fix};
        else return {GAT_K(edge_fwd2_kernel<HD, D, N2, BF, true, true>), 64, 1, fix};
    }
    if (ext) {
        if constexpr (N3 != 0) return {GAT_K(edge_fwd3_kernel<HD, D, N3, BF, true>), 64, G3, fix};
        else return {GAT_K(edge_fwd2_kernel<HD, D, N2, BF, true>), 64, 1, fix};
    }
    if (!packed_layout()) return {GAT_K(edge_fwd_kernel<HD, D, false, BF>), 256, 4, fix};
    const int wpb = fwd_waves();                                                  // two or four channels per lane (see edge_fwd2_kernel)
    if constexpr (N3 != 0) {                                                      // group-per-row kernel (GAT_ROWGROUP=0: the chunked one, A/B)
        if (row_groups()) return {GAT_K(edge_fwd3_kernel<HD, D, N3, BF>), 64u * wpb, G3 * wpb, fix};
    }
    if constexpr (N2 == 4) {
        if (lane_channels() == 4) return {GAT_K(edge_fwd2_kernel<HD, D, 4, BF>), 64u * wpb, wpb, fix};
    }
    return {GAT_K(edge_fwd2_kernel<HD, D, 2, BF>), 64u * wpb, wpb, fix};
}

// Backward.  store: message rows or records by CSC slot (else atomics into gPL); taps: the parity form that also writes ge / galpha;
// stash: per-edge records + pull pass instead of message rows.  Attention dropout / DropEdge (drop) exist for the store path only,
// as the DROP instantiation of the kernel the default settings pick; the A/B switches do not apply to them.
// dbg (experiment library only, GAT_DBG): timing variants, most with WRONG results; 0 = the product kernel of the selection.
// pe (edge features, always with drop): the PE instantiation of the same DROP kernel.
template <int HD, int D, bool BF>
EdgePick parent_pick_bwd(const EdgeBwdArgs& a, bool drop, int dbg, bool pe) {
    constexpr int N3 = stash_n<HD, D>(), N2 = (HD >= 32 && D % 4 == 0) ? 4 : 2;
    const bool store = a.pos != nullptr && a.msg != nullptr, taps = a.ge != nullptr, stash = a.stash != nullptr && !taps;
    // records in CSR edge order (EdgeBwdArgs::edge_order, set under records_take_edge_order): the EO instantiation of the group-per-row
    // record kernel, plain / DROP / PE; launch_edge_backward refuses the flag where that kernel is not the pick
    [[maybe_unused]] const bool eo = a.edge_order != 0 && stash && store && !BF && N3 != 0 && row_groups() && dbg == 0;
    [[maybe_unused]] const bool lines = eo && stash_lines();
    if (drop) {
        if (!store) return {};
        if (pe) {
            if (taps) return {GAT_K(edge_bwd_kernel<HD, D, true, true, 0, BF, true, true>)};
            if constexpr (N3 != 0 && !BF) {
                if (lines) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, false, false, true, true, true, true>)};
                if (eo) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, false, false, true, true, true>)};
            }
            if constexpr (N3 != 0) return {stash ? GAT_K(edge_bwd3_kernel<HD, D, N3, 0, BF, false, true, true>) : GAT_K(edge_bwd3_kernel<HD, D, N3, 0, BF, true, true, true>)};
            else return {GAT_K(edge_bwd2_kernel<HD, D, N2, 0, BF, false, true, true>)};
        }
        if (taps) return {GAT_K(edge_bwd_kernel<HD, D, true, true, 0, BF, true>)};
        if constexpr (N3 != 0 && !BF) {
            if (lines) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, false, false, true, false, true, true>)};
            if (eo) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, false, false, true, false, true>)};
        }
        if constexpr (N3 != 0) return {stash ? GAT_K(edge_bwd3_kernel<HD, D, N3, 0, BF, false, true>) : GAT_K(edge_bwd3_kernel<HD, D, N3, 0, BF, true, true>)};
        else return {GAT_K(edge_bwd2_kernel<HD, D, N2, 0, BF, false, true>)};
    }
    const bool msg_rows = store && !taps && packed_layout();                      // packed message-row kernels
#ifdef GAT_EXPERIMENTS
    if constexpr (HD == 64 && D == 8) {
        if (store && !taps && !stash) {                                           // GAT_DBG=1: no message store, 2: sequential slots
            if (dbg == 1) return {GAT_K(edge_bwd_kernel<HD, D, true, false, 1>)};
            if (dbg == 2) return {GAT_K(edge_bwd_kernel<HD, D, true, false, 2>)};
        }
        if (stash && !BF && row_groups()) {
            // GAT_DBG=1: no record store, 2: records in CSR order, 3; 9: double walk; scatter folded into 64 MiB (10), 16 MiB, 4 MiB,
            // 1 MiB (13), 1 GiB (14); 64 (15), 512, 4,096, 32,768 (18) sequential write fronts
            if (const void* fn = bwd3_dbg<1, 2, 3, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18>(dbg)) return {fn};
            // wave-specialised stores.  4: 7 + 1 waves, 512-thread blocks — half as many are resident as of the 256-thread product
            // kernel the grid is sized from, so half its grid
            if (dbg == 4) return {GAT_K(edge_bwd4_kernel<7, 4>), 512, 4, nullptr, 2};
            if (dbg == 5) return {GAT_K(edge_bwd4_kernel<3, 4>)};                 // 3 + 1 waves
            if (dbg == 6) return {GAT_K(edge_bwd4_kernel<3, 4, 1>)};              // 3 + 1 waves, sc1 stores
            if (dbg == 7) return {GAT_K(edge_bwd4_kernel<3, 4, 2>)};              // sc0 sc1
            if (dbg == 8) return {GAT_K(edge_bwd4_kernel<3, 4, 3>)};              // nt
        } else if (stash && !BF) {
            if (dbg == 1) return {GAT_K(edge_bwd2s_kernel<64, 8, 4, 1>)};
            if (dbg == 2) return {GAT_K(edge_bwd2s_kernel<64, 8, 4, 2>)};
        }
    }
#endif
    if constexpr (N3 != 0) {
        if constexpr (!BF) {
            if (lines) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, false, false, false, false, true, true>)};
            if (eo) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, false, false, false, false, true>)};
        }
        // records; bf16 storage: always the group-per-row kernel (GAT_ROWGROUP=0 has no bf16 form)
        if (stash) return {(BF || row_groups()) ? GAT_K(edge_bwd3_kernel<HD, D, N3, 0, BF>) : GAT_K(edge_bwd2s_kernel<HD, D, N3>)};
        // message rows from the group-per-row kernel.  Both switches are read, GAT_GROUP_MSG first: a process that sets both reports
        // both in gat_switches() (either one at 0 gives the wave-per-row kernel)
        if (const bool gm = group_msg(); msg_rows && row_groups() && gm) {
#ifdef GAT_EXPERIMENTS      // GAT_DBG=1 on a message-row layer (BASELINE config 5): the walk without its message-row stores — WRONG RESULTS, timing / PMC
            if constexpr (HD == 32 && D == 8 && BF) {     // attribution only (DESIGN §4 "Round 4": how much of the backward's reads is fill for its 64-byte row writes)
                if (dbg == 1) return {GAT_K(edge_bwd3_kernel<HD, D, N3, 1, true, true>)};
            }
#endif
            return {GAT_K(edge_bwd3_kernel<HD, D, N3, 0, BF, true>)};
        }
    }
    if (msg_rows) {
        if constexpr (N2 == 4) {
            if (lane_channels() == 4) return {GAT_K(edge_bwd2_kernel<HD, D, 4, 0, BF>)};
        }
        return {GAT_K(edge_bwd2_kernel<HD, D, 2, 0, BF>)};
    }
    return {store ? (taps ? GAT_K(edge_bwd_kernel<HD, D, true, true, 0, BF>) : GAT_K(edge_bwd_kernel<HD, D, true, false, 0, BF>))
                  : (taps ? GAT_K(edge_bwd_kernel<HD, D, false, true, 0, BF>) : GAT_K(edge_bwd_kernel<HD, D, false, false, 0, BF>))};
}
