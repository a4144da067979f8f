// mrz_seq_stats.h -- the diagnostic counters of mrz_seq_state.prof (-DMRZ_SEQ_STATS / -DMRZ_SEQ_PROFILE builds): ONE list
// for the sequencers' indices (MRZ_ST_*) and the names MRZ_PRINT_PROF prints them under (mrz_capi.hip).  Host and device.
#pragma once
#include "mrz_common.h"

// X(identifier, printed name), in the order of the slots of prof[]
#define MRZ_SEQ_STATS_LIST(X) \
    X(BATCHES, "batches") X(FORMED, "formed") X(COMMITTED, "committed") X(SEGMENTS, "segments") \
    X(EMITS, "emits") X(BACKJUMP, "backjump") X(REWALK, "rewalk") X(LONGRES, "longres") X(SEQ, "seq_cands") \
    X(CUT_CPLX, "cut_cplx") X(CUT_OVERFLOW, "cut_overflow") X(SKIPOUT, "skipout") X(CONF0, "conf0") \
    X(PAIRS, "pairs") X(T_FORM, "t_form") X(T_WALK, "t_walk") X(T_CONF, "t_conf") X(T_PAIRS, "t_pairs") \
    X(T_LOOP, "t_loop") X(T_REWALK, "t_rewalk") X(T_LONG, "t_long") X(T_SEQ, "t_seq") X(FARMED, "farmed") \
    X(L_POST, "l_post") X(L_STRIPE, "l_stripe") X(L_BWD, "l_bwd") X(L_WAIT, "l_wait") X(L_ROUNDS, "l_rounds") \
    X(F_POST, "f_post") X(F_WAIT, "f_wait") X(F_FOLD, "f_fold") X(S_TAB, "s_tab") X(S_PAIR, "s_pair") \
    X(S_INS, "s_ins") X(OVL, "ovl") X(OVL_OK, "ovl_ok") X(X_WALK, "x_walk") X(X_CASC, "x_casc") \
    X(X_POOL, "x_pool") X(X_WIN, "x_win") X(X_SAME, "x_same") X(C_WIN, "c_win") X(C_EVICT, "c_evict") \
    X(C_DEEP, "c_deep") X(C_MANY, "c_many") X(C_FAIL, "c_fail") X(C_TIE, "c_tie") X(C_NW, "c_nw") \
    X(T_OVL, "t_ovl") X(H_PRE, "h_pre") X(H_CAND, "h_cand") X(H_POST, "h_post") X(T_SCAN, "t_scan") \
    X(T_FOLD, "t_fold") X(T_COMMIT, "t_commit") X(REPREP, "reprep") X(W_STALE, "w_stale") X(W_DROP, "w_drop") \
    X(RESET, "reset") X(T_TURN, "t_turn") X(T_PREP, "t_prep") X(T_PRECOMMIT, "t_precommit") X(E_MASK, "e_mask") \
    X(E_CULL, "e_cull") X(E_XW, "e_xw") X(E_INWIN, "e_inwin") X(E_WINDOW, "e_window") X(E_BULK, "e_bulk") \
    X(E_MORE, "e_more") X(T_PC_CW, "t_pc_cw") X(T_PC_LOG, "t_pc_log") X(T_PC_BEST, "t_pc_best") \
    X(T_PC_BULK, "t_pc_bulk") X(T_TURNWORK, "t_turnwork") X(T_SNAP, "t_snap") X(REBULK, "rebulk") \
    /* (the narrow engine's own) */ \
    X(BATCH_LANES, "batch_lanes") X(CUT_LONG, "cut_long") X(CUT_WALK, "cut_walk") \
    X(CUT_CONFLICT, "cut_conflict") X(CUT_CULL, "cut_cull") X(BATCH_EMITS, "batch_emits") \
    X(CUT_CASCADE, "cut_cascade") X(BATCH_FORMED, "batch_formed") X(T_WALK2, "t_walk2") X(T_SCANS, "t_scans") \
    X(T_CONFLICT, "t_conflict") X(T_WINDOW, "t_window") \
    /* (the deep engine's own) */ \
    X(D_BATCHES, "d_batches") X(D_LANES, "d_lanes") X(D_ROUNDS, "d_rounds") X(D_RESCANNED, "d_rescanned") \
    X(D_COOP, "d_coop") X(D_T_FORM, "d_t_form") X(D_T_SCAN, "d_t_scan") X(D_T_COMMIT, "d_t_commit") \
    X(D_T_RESCAN, "d_t_rescan") X(D_T_TOTAL, "d_t_total") X(D_LAUNCHES, "d_launches") X(D_T_COOP, "d_t_coop") \
    X(D_COOP_REC, "d_coop_rec") X(D_RESOLVED, "d_resolved") X(D_S_COOP, "d_s_coop") \
    X(D_S_CONFLICT, "d_s_conflict") X(D_S_CULLED, "d_s_culled") X(D_S_NOCULL, "d_s_nocull") \
    X(D_S_STALE, "d_s_stale") X(D_C_OVER_ALT, "d_c_over_alt") X(D_C_OVER_NOALT, "d_c_over_noalt") \
    X(D_C_EMPTY, "d_c_empty") X(D_C_DISPLACE, "d_c_displace") X(D_C_OTHER, "d_c_other") \
    /* (the split of d_t_scan -- committer: post the job, scan its own share, wait for the helpers, copy their records in; \
       the scan helper with ticket 0: from the poll's match to the end of its acquire, read the job, scan, records out + signal; \
       of its wave 0's walks: from issuing a group's loads to the end of the wait before its fold, and the folds) */ \
    X(D_T_POST, "d_t_post") X(D_T_OWN, "d_t_own") X(D_T_WAIT, "d_t_wait") X(D_T_COPYIN, "d_t_copyin") \
    X(DH_T_ACQ, "dh_t_acq") X(DH_T_JOB, "dh_t_job") X(DH_T_SCAN, "dh_t_scan") X(DH_T_OUT, "dh_t_out") \
    X(DH_T_LDWAIT, "dh_t_ldwait") X(DH_T_FOLD, "dh_t_fold")

#define MRZ_ST_ENUM(id, name) MRZ_ST_##id,
enum { MRZ_SEQ_STATS_LIST(MRZ_ST_ENUM) MRZ_ST_N };
#undef MRZ_ST_ENUM
static_assert(MRZ_ST_N <= (int)(sizeof(((mrz_seq_state *)0)->prof) / sizeof(int64_t)), "mrz_seq_state.prof holds the counters");
