/*
 * dpemu.h -- C ABI of the MI355X-native batched QubiC distributed-processor
 * emulator (libdpemu.so).
 *
 * The emulator executes the 128-bit machine code that distproc's assembler
 * writes into cmd_mem (python/distproc/assembler.py:341-429,623-641) across
 * many (shot, core) lanes, cycle-exact against the gateware:
 *   proc core           hdl/proc.sv:9-171, ctrl.v:55-595, alu.v, instr_ptr.v,
 *                       qclk.v, reg_file.v, cmd_mem.v (READ_LATENCY=3)
 *   pulse emission      hdl/pulse_reg.sv:16-107, pulse_iface.sv
 *   measurement fproc   hdl/fproc_meas.sv, fproc_lut.sv, core_state_mgr.sv,
 *                       meas_lut.sv
 *   sync barrier        hdl/sync_iface.sv + ctrl.v:347-363,510-552 (the
 *                       controller itself is build-defined)
 * and synthesises DDS I/Q samples from the pulse events (build-defined DDS).
 *
 * Each entry point replaces one piece of the reference simulation path
 * (SURVEY.md §8b): the cocotb/Verilator harness of toplevel_sim
 * (sim_modules/toplevel_sim.sv:13-33; cocotb/proc/test_proc.py:29-38 loads
 * cmd_mem, drives reset/fproc/sync, samples pulse_iface every clock).
 *
 * Conventions: return 0 on success, a negative DPEMU_E* code on failure (no
 * exceptions cross the ABI; dpemu_last_error() has the message).  Caller
 * owns every pointer it passes.  Device-pointer outputs must be device
 * memory of the context's device; NULL skips that output.  A context is not
 * re-entrant (one host thread at a time); use one per device (one process
 * per GPU).  Work a context enqueues runs in call order even across streams:
 * a call on a stream other than the previous call's first makes that stream
 * wait for the previous call's work (the context's scratch buffers and
 * uploaded constants are shared by its calls).
 */
#ifndef DPEMU_H
#define DPEMU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPEMU_ABI_VERSION 8

/* ---- error codes ---------------------------------------------------- */
#define DPEMU_OK            0
#define DPEMU_E_INVALID   (-22)   /* bad argument / inconsistent config  */
#define DPEMU_E_NOMEM     (-12)   /* device allocation failed            */
#define DPEMU_E_DEVICE     (-5)   /* HIP runtime error                   */
#define DPEMU_E_NOPROG     (-2)   /* run before load_programs            */

/* ---- lane terminal status (summary.w1 bits 23:16) -------------------- */
#define DPEMU_ST_DONE        1    /* decoded DONE (1010) or opcode 0000 (ctrl.v:365-397) */
#define DPEMU_ST_MAX_CYCLES  2    /* next decode, or a wait's end, beyond max_cycles     */
#define DPEMU_ST_HUNG_OPCODE 3    /* opcode[7:4] in 1101..1111: DECODE forever (ctrl.v:399-414) */
#define DPEMU_ST_DEADLOCK    4    /* sync / fproc wait that can never complete           */

/* ---- lane flags (summary.w1 bits 31:24) ------------------------------ */
#define DPEMU_F_LATE          0x01 /* trig/idle decoded after cmd_time: waits for qclk wrap */
#define DPEMU_F_EVENT_OVF     0x02 /* more events than event_cap (count still exact)        */
#define DPEMU_F_TRACE_OVF     0x04 /* more register-trace records than trace_cap            */
#define DPEMU_F_MEAS_OVF      0x08 /* more measurements than meas_cap                       */
#define DPEMU_F_DOUBLE_STROBE 0x10 /* trig at the first decode with cmd_time 0: the reset
                                      hold keeps qclk at 0 two cycles -> two cstrobes      */
#define DPEMU_F_GUARD         0x20 /* internal error: interpreter iteration guard tripped    */

/* ---- fproc back ends --------------------------------------------------*/
#define DPEMU_FPROC_MEAS 0        /* hdl/fproc_meas.sv: latest stored bit, ready at D+2   */
#define DPEMU_FPROC_LUT  1        /* hdl/fproc_lut.sv: id==0 wait own meas, else LUT      */

/* ---- event kinds (event.w2 bits 31:28) ------------------------------- */
#define DPEMU_EV_STROBE      0    /* pulse_iface.cstrobe high: pulse register snapshot    */
#define DPEMU_EV_PULSE_RESET 1    /* pulse_iface.reset high (PULSE_RESET decode cycle)    */

/* ---- register-trace pseudo addresses ---------------------------------- */
#define DPEMU_TRACE_QCLK_LOAD 16  /* INC_QCLK loaded qclk (value = qclk at t)             */
#define DPEMU_TRACE_QCLK_RST  17  /* SYNC reset qclk (value 0 at t)                       */

/* execution knobs (dpemu_config.exec_flags): results never depend on them; the
 * parity tests run every variant against the oracle */
#define DPEMU_X_PROG_LDS    0x1   /* run non-pulse-only programs on the general interpreter with each
                                     workgroup's programs staged in LDS when they fit */
#define DPEMU_X_HIST_DIRECT 0x4   /* outcome histogram: atomics straight into out->hist       */
#define DPEMU_X_HIST_REPL   0x8   /* outcome histogram: privatised replicas + reduce          */
#define DPEMU_X_PROG_MAJOR  0x10  /* fetch from the program-major image, not the command-major copy */
#define DPEMU_X_GENERAL     0x20  /* run every program on the general interpreter (interp_kernel) */
#define DPEMU_X_MACRO_DIRECT 0x40 /* branch-free register programs: per-lane macro fetch (macro_kernel),
                                     not the LDS-staged program chunks (macro_staged_kernel) */
#define DPEMU_X_STREAM_EVENTS 0x80 /* cache hint: branch-free register programs store their event rows
                                     nontemporal (whole-wave stores; others write-back), in macro_kernel
                                     and macro_staged_kernel alike.  Workload-
                                     dependent: config 4 two-qubit RB -9 %, RB-shaped programs +10 %
                                     (profiles/r06_stpol_ab.json) */

#define DPEMU_MAX_CORES 64
#define DPEMU_MEAS_LOOKUP 16      /* a core's first 16 measurements are visible to fproc;
                                     later ones set DPEMU_F_MEAS_OVF and are invisible  */
#define DPEMU_LUT_FIRE_CAP 16     /* meas_lut fires recorded per shot (later fires lost) */

/*
 * Timebase: cycle t = 0 is the first DECODE after reset.  qclk(0) = qclk(1) = 0
 * (reset hold, proc.sv:125-136), qclk(t) = t - 1 afterwards until INC_QCLK or
 * SYNC reload it.  All times are emulated fabric clocks (2 ns at 500 MHz).
 */
typedef struct dpemu_config {
    uint32_t cores_per_shot;   /* C: power of two, 1..64; lane = shot*C + core        */
    uint32_t n_groups;         /* program groups; group(s) = (s/shots_per_group)%n_groups */
    uint32_t shots_per_group;  /* >= 1                                                  */
    uint32_t max_cycles;       /* <= 2^31 - 64                                          */
    uint32_t event_cap;        /* event slots per lane (<= DPEMU_MAX_EVENT_CAP)           */
    uint32_t trace_cap;        /* register-trace slots per lane (0 = no trace; <= DPEMU_MAX_EVENT_CAP) */
    uint32_t meas_cap;         /* measurement slots per lane (<= 32)                     */
    uint32_t fproc_mode;       /* DPEMU_FPROC_*                                          */
    uint32_t meas_elem;        /* strobe with (cfg & 3) == meas_elem is a readout; 0xFF none */
    uint32_t meas_latency;     /* readout strobe -> meas_valid, clocks (>= 1)           */
    uint32_t sync_latency;     /* last sync enable -> sync.ready, clocks (>= 1)         */
    uint32_t exec_flags;       /* DPEMU_X_* execution knobs (results never depend on them) */
    uint64_t sync_mask;        /* participant cores (bit c); 0 = all C cores.  Bits at or above C name no
                                  core and are ignored.  A nonzero word with no bit below C leaves no
                                  participant: no barrier completes and every SYNC ends in DEADLOCK.  A
                                  core outside the mask that executes SYNC never gets ready (DEADLOCK) */
    uint64_t seed;             /* Philox4x32-10 key                                      */
    uint32_t lut_mask;         /* meas_lut mask (nonzero), meas_lut.sv:16: the cores (bit c) whose
                                  meas_valid the LUT waits for.  Bits at or above C are NOT ignored: no
                                  such core ever measures, so the LUT never fires and every fproc_lut
                                  read with a nonzero id ends in DEADLOCK                              */
    uint32_t meas_model;       /* DPEMU_MEAS_STATE: outcome = prepared state; DPEMU_MEAS_READOUT:
                                  the discriminated readout signal (ro_* below)            */
    uint32_t p1_threshold[DPEMU_MAX_CORES]; /* P(state=1) = thr/2^32; 0xFFFFFFFF = always 1 */
    uint64_t lut_table[256];   /* meas_lut table: lut_out = table[addr], bit c -> core c */
    /* readout model (meas_model = DPEMU_MEAS_READOUT), per readout strobe with amp word A:
     *   z = Irwin-Hall(4) of the 16-bit halves of Philox words 1, 2, minus 131070
     *   x = (state ? +1 : -1) * ((ro_sep * A) >> 16) + ((z * ro_sigma) >> 16)   (int64)
     *   outcome = x > ro_thr
     * with ro_win != 0 the separation also scales with the readout window:
     *   s = (s * (min(W, ro_win) * floor(2^24 / ro_win))) >> 24   (int64)
     * unless W == 0: a CW envelope word (length field 0) plays until the next
     * pulse, so it integrates the whole window and s is not scaled
     * W = the strobe's envelope-length field (env word bits 23:12, in env words)
     * -- a window shorter than ro_win integrates less signal                  */
    int32_t  ro_sep;           /* half the state separation at full readout amplitude    */
    uint32_t ro_sigma;         /* noise scale, Q16 (noise sigma = ro_sigma / 2^16 * 37837.6) */
    int32_t  ro_thr;           /* discriminator threshold                                */
    uint32_t ro_win;           /* reference readout window (env words, < 4096); 0 = amplitude only */
    uint32_t hist_assign;      /* 0: out->hist += this run's counts; 1: out->hist = this run's
                                  counts (no separate zeroing launch before each run)        */
    uint32_t lane_order;       /* DPEMU_LANES_CORE_MAJOR (0) or DPEMU_LANES_SHOT_MAJOR (1), below */
    /* readout demodulation model (meas_model = DPEMU_MEAS_DEMOD, ABI 8).
     * The return of the lane's latest readout-drive strobe (cfg & 3 == ro_drv_elem,
     * t_d <= t_lo) is mixed with the readout strobe's own LO (cfg & 3 == meas_elem,
     * at t_lo) and accumulated per clock over their overlap; both phases follow the
     * DDS phase accumulator, F * (k - t_ref) + phase17 << 15 (t_ref = the latest
     * pulse_reset <= t_lo; F = the 32-bit frequency word of the pulse's freq index,
     * dpemu_load_readout_freqs).  Per clock k of the overlap, with s the prepared state:
     *   return  amp_d * ro_gain[s] / 2^16 at phase F_d (k - ro_delay - t_ref)
     *           + phase_d << 15 + ro_theta[s]
     *   acc    += return * conj(LO)   (int32 I / Q, closed form: exact integer
     *                                   arithmetic of DESIGN.md §2, oracle/readout.c)
     *   acc    += noise: (z_I, z_Q) * ro_sigma / 2^16 (Hadamard pairs of 4 Philox halves)
     *   x       = (acc_I * axis_I + acc_Q * axis_Q) >> 15, axis = ro_axis[core]
     *   outcome = x > ro_thr, meas_valid at max(t_lo + window + meas_latency,
     *             the lane's previous meas_valid + 1)   (an in-order readout pipeline)
     * window = the readout strobe's env length field (bits 23:12) * ro_cpw clocks
     * (length 0: a CW envelope, 4096 words); the drive pulse lasts likewise.
 * This closed form is the flat-top (drive envelope 32767 throughout), unit-LO,
 * one-term-per-clock case of dpemu_demod_iq below, which accumulates the same
 * {I, Q} from the synthesised waveforms: the two agree within 2.2e-3 |acc| + 64
 * on such pulses (tests/test_demod_iq.py).                        */
    uint32_t ro_drv_elem;      /* element of the readout drive (rdrv) strobes, 0..3, != meas_elem */
    uint32_t ro_cpw;           /* clocks per env word of the rdrv / rdlo pulses, 1..8 (4 for
                                  channel_config.json's rdrv 16 samples/clk interp 16, rdlo 4 / 4) */
    uint32_t ro_delay;         /* drive -> ADC return delay, clocks (< 2^20)                */
    uint32_t ro_theta[2];      /* return phase shift for prepared state 0 / 1 (2^32 = 2 pi)  */
    uint32_t ro_gain[2];       /* return amplitude for state 0 / 1, Q16 (<= 65536)         */
    uint32_t ro_axis[DPEMU_MAX_CORES]; /* discriminator axis per core, Q15: I16 low | Q16 high */
} dpemu_config;

#define DPEMU_MEAS_STATE   0
#define DPEMU_MEAS_READOUT 1
#define DPEMU_MEAS_DEMOD   2      /* rdlo demodulation of the rdrv return (ro_drv_elem ...) */
#define DPEMU_RO_CPW_MAX   8      /* ro_cpw bound: an accumulation window is <= 2^15 clocks   */

/* lane order of every per-lane output (dpemu_config.lane_order) */
#define DPEMU_LANES_CORE_MAJOR 0  /* lane = core * n_shots + (shot - shot_begin)                  */
#define DPEMU_LANES_SHOT_MAJOR 1  /* lane = (shot - shot_begin) * C + core: a shot's cores adjacent */

#define DPEMU_MAX_EVENT_CAP (1u << 20)   /* event / trace slots per lane (validate)  */

/*
 * Lanes: lane L = core * n_shots + (shot - shot_begin) -- core-major, so the
 * lanes of one core's shots are adjacent (the lanes that run one program in
 * lockstep write whole cache lines) -- or, with lane_order SHOT_MAJOR,
 * L = (shot - shot_begin) * C + core (a shot's cores adjacent: the layout the
 * fproc / sync interpreter writes as whole lines, since a wave holds whole
 * shots).
 *
 * Per-lane summary, 8 x u32:
 *   w0 t_end      decode cycle of DONE (done_gate from t_end+1) or of the stop
 *   w1 ip[15:0] | status[23:16] | flags[31:24]
 *   w2 n_events   strobe + pulse_reset events (may exceed event_cap)
 *   w3 n_instr    instructions decoded (DONE included)
 *   w4 qclk_end   qclk at t_end
 *   w5 n_meas     measurements taken
 *   w6 meas_bits  outcome of measurement m in bit m (m < 32)
 *   w7 n_trace    register-trace records (may exceed trace_cap)
 *
 * Event (slot-major: slot k of lane L at index k*n_lanes + L), one 16-B record
 * per pulse_iface strobe (hdl/pulse_iface.sv:2-6) or pulse reset:
 *   uint4 {t, env[23:0] | cfg<<24 | kind<<28, phase[16:0] | freq<<17, amp[15:0]}
 * (qclk at an event follows from t and the lane's qclk loads / resets, which
 * the register trace records)
 * Trace (slot-major): uint4 {t (first cycle the value is visible), addr, value, 0}
 * Meas  (slot-major): uint2 {valid cycle, bit}
 * Histogram: uint64 [n_groups][2^C] (C <= 12), key bit c = last outcome of core c.
 */
typedef struct dpemu_outputs {
    uint32_t *summary;    /* [n_lanes][8]                      */
    uint32_t *events;     /* [event_cap][n_lanes][4]           */
    uint32_t *trace;      /* [trace_cap][n_lanes][4]           */
    uint32_t *meas;       /* [meas_cap][n_lanes][2]            */
    uint32_t *regs;       /* [16][n_lanes] final register file */
    uint64_t *hist;       /* [n_groups][2^C], accumulated (or assigned: hist_assign) */
    uint64_t *hist_next;  /* optional, dpemu_run only: a second [n_groups][2^C] buffer, disjoint
                             from hist, that this run sets to zero in passing -- the buffer the
                             caller's next run accumulates into, so a pipeline of runs rotating
                             over three histogram buffers needs no zeroing launch (ABI 7) */
    int32_t  *acc;        /* [meas_cap][n_lanes][2] accumulated {I, Q} of each readout (the
                             accbuf of hwconfig.py:128,138-140); DEMOD runs only (ABI 8) */
} dpemu_outputs;

typedef struct dpemu_ctx dpemu_ctx;

/* Library / device --------------------------------------------------- */
int         dpemu_abi_version(void);
/* sizeof(dpemu_config), sizeof(dpemu_outputs), sizeof(dpemu_dds_channels) as
 * this library was compiled: a binding compares them with its own layout
 * before the first call (the version number alone does not catch a build
 * from a half-edited header).  out: 3 entries. */
int         dpemu_struct_sizes(uint64_t *out);
int         dpemu_create(int device, dpemu_ctx **out);
int         dpemu_destroy(dpemu_ctx *ctx);
const char *dpemu_last_error(dpemu_ctx *ctx);

/*
 * Programs: n_programs cmd_mem images.  `words` holds n_cmds little-endian
 * u128 commands as u32 quads (word i of the u128 = bits [32i+31:32i],
 * cmd_mem_iface.sv:19-21), i.e. 4 * n_cmds u32 words; program p starts at
 * COMMAND offsets[p] with n_instr[p] commands (assembler cmd_buf bytes
 * reinterpret directly).  n_cmds, offsets and n_instr all count 16-byte
 * commands; offsets[p] + n_instr[p] <= n_cmds for every p, else
 * DPEMU_E_INVALID (nothing past the caller's 16 * n_cmds bytes is read).  Fetch beyond
 * n_instr reads 0 (= DONE), as the zero-initialised 2^16-deep cmd_mem of
 * toplevel_sim does.  prog_table[g*C + c] = program run by core c of shots
 * in group g.  Replaces load_commands (cocotb/proc/test_proc.py:29-38).
 */
int dpemu_load_programs(dpemu_ctx *ctx, const uint32_t *words, uint64_t n_cmds, const uint32_t *offsets,
                        const uint32_t *n_instr, uint32_t n_programs,
                        const uint32_t *prog_table, uint32_t n_groups, uint32_t cores_per_shot);

/*
 * Frequency words of the DEMOD readout model (ABI 8), per loaded program p:
 * the readout drive element's freq index i reads words[drv_off[p] + i] when
 * i < drv_len[p], else 0; the LO element's reads words[lo_off[p] + i] (i <
 * lo_len[p]).  Each word is entry i's first word of the element's
 * freq_buffer, f / f_clk * 2^32 (python/distproc/asmparse.py:64-86; the
 * assembler's freq_buffers, assembler.py:510-516).  Arrays hold n_programs
 * entries (the count of the last dpemu_load_programs); offsets + lengths
 * must stay within n_words.  dpemu_load_programs clears the tables, and a
 * DEMOD run without them is DPEMU_E_INVALID.
 */
int dpemu_load_readout_freqs(dpemu_ctx *ctx, const uint32_t *words, uint64_t n_words, const uint32_t *drv_off,
                             const uint32_t *drv_len, const uint32_t *lo_off, const uint32_t *lo_len);

/* Emulate shots [shot_begin, shot_begin + n_shots) on `stream` (hipStream_t or
 * NULL).  n_lanes = n_shots * C.  Outputs are device pointers.  out->hist_next,
 * when set, is zeroed even for n_shots = 0; overlapping out->hist is
 * DPEMU_E_INVALID. */
int dpemu_run(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
              const dpemu_outputs *out, void *stream);

/*
 * dpemu_run with the prepared state of every readout supplied by the caller
 * (ABI 8, additive): the interpreter half of the co-simulation loop (DESIGN.md
 * §2 "Co-simulation"; the qubit half is dpemu_qsim_meas below).  This comment is
 * the normative definition.
 *
 *   states == NULL   the call is dpemu_run exactly: same plan, same kernel,
 *                    same bytes, same dpemu_last_kernel
 *   states != NULL   wherever dpemu_run draws a readout's prepared state --
 *                    Philox word 0 of (seed, shot, core, m) against
 *                    p1_threshold[core] -- the state of readout m of a lane is
 *                      m < 32 ? (states[lane] >> m) & 1 : 0
 *                    with lanes in the run layout of cfg->lane_order:
 *                    dpemu_qsim_meas's buffer of the same run is passed as it
 *                    is.  p1_threshold is not read
 *   DPEMU_MEAS_STATE    the outcome is that bit; no Philox call is made
 *   DPEMU_MEAS_READOUT  the bit replaces `state` in x = +-s + noise; the noise
 *                    draw (words 1, 2 of the same counter) is untouched
 *   everything else  is dpemu_run's: timing, meas_valid, the event, trace and
 *                    meas records, registers, flags, the histogram, hist_next
 *
 * DPEMU_E_INVALID, before any launch: everything dpemu_run refuses; states not
 * 4-byte aligned; meas_model DPEMU_MEAS_DEMOD with states != NULL (the *_st
 * readout stages below take the states of a DEMOD chain post hoc).  n_shots 0
 * behaves as dpemu_run and states is not touched.
 *
 * Every program runs on branch_kernel -- pulse-only, branch-free and branching
 * programs alike, in every fproc_mode: the route DEMOD runs take -- and the
 * exec_flags that pick other kernel families are ignored (results never depend
 * on them).  dpemu_last_kernel reports the variant with feature bit 0x80, e.g.
 * "branch_kernel<feat=0x8b,c8>"; the timing pair is recorded around the kernel
 * as for dpemu_run.  `states` is a device pointer to n_shots * C words, read
 * once per lane.
 */
int dpemu_run_states(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
                     const dpemu_outputs *out, const uint32_t *states /* device [n_lanes], nullable */,
                     void *stream);

/* Same, with host output pointers (the library stages device buffers);
 * host_out->hist_next must be NULL (DPEMU_E_INVALID otherwise). */
int dpemu_run_host(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin,
                   uint64_t n_shots, const dpemu_outputs *host_out);

/*
 * DDS synthesis (build-defined fixed point; CPU restatement
 * oracle/dds_ref.c).  One channel = one (lane, element) pair: it plays the
 * lane's strobes whose cfg & 3 == element, with the lane's pulse_resets as
 * phase references, from the events dpemu_run wrote (slot-major, n_lanes
 * stride, count = min(summary n_events, event_cap)).  Env / freq tables are
 * the assembler's env_buffers / freq_buffers (asmparse.py:46-86 formats),
 * concatenated; channel c reads env words [env_off, env_off + env_len) and
 * freq words [freq_off, freq_off + freq_len).  Output: iq[c][n_samples] of
 * int16 {I, Q} pairs; sample j is at emulated cycle j / spc.
 *
 * The dpemu_dds_channels arrays are HOST memory (n_channels entries each);
 * summary / events / env_tables / freq_tables / iq_out are device pointers.
 * n_samples must be a multiple of 4; event_cap <= 1024.
 */
typedef struct dpemu_dds_channels {
    uint32_t n_channels;
    uint32_t n_lanes;          /* stride of the event arrays (dpemu_run's n_lanes) */
    uint32_t n_samples;        /* samples per channel                               */
    uint32_t event_cap;        /* event slots per lane of the event arrays          */
    const uint32_t *ch_lane;   /* lane of each channel                               */
    const uint32_t *ch_elem;   /* element (cfg & 3) of each channel                  */
    const uint32_t *spc;       /* samples per clock, 1..16                           */
    const uint32_t *interp;    /* output samples per envelope sample, >= 1           */
    const uint32_t *env_off;
    const uint32_t *env_len;
    const uint32_t *freq_off;
    const uint32_t *freq_len;
} dpemu_dds_channels;

int dpemu_dds(dpemu_ctx *ctx, const dpemu_dds_channels *ch, const uint32_t *summary,
              const uint32_t *events, const uint32_t *env_tables, const uint32_t *freq_tables,
              int16_t *iq_out, void *stream);

/* The Q15 sine table both the DDS kernel and its CPU restatement use. */
int dpemu_dds_sin_lut(int16_t *out4096);

/*
 * Waveform demodulation (ABI 8, additive): the accumulated {I, Q} of every
 * readout from the SYNTHESISED drive and LO waveforms -- what the rdlo DDS
 * times the ADC return accumulates into accbuf (hwconfig.py:128,138-140) --
 * where the DEMOD model above evaluates a flat-top closed form.  A pair is one
 * lane's drive channel (element ro_drv_elem) and LO channel (element
 * meas_elem), rows of dpemu_dds outputs (words {I16 low, Q16 high}).
 *
 *   readouts  the lane's strobe events with cfg & 3 == meas_elem among its
 *             first min(n_events, event_cap) events, in event order; the m-th
 *             is readout m, m >= meas_cap is dropped
 *   window    strobe at t_lo with env word pe: clocks [t_lo, t_lo + W ro_cpw),
 *             W = pe bits 23:12 (0: 4096); LO samples j = n spc_lo + k of those
 *             clocks n, clipped to n_samples_lo
 *   ADC       at LO sample (n, k): the drive row's sample (n - ro_delay) spc_drv
 *             + k (spc_drv / spc_lo), or 0 when n < ro_delay or the index is
 *             >= n_samples_drv (spc_lo a power of two, spc_drv a multiple of it)
 *   state     s = Philox word 0 of (seed, global shot, core, m) < p1_threshold[core]
 *             (or a threshold of 0xFFFFFFFF): the DEMOD model's draw
 *   return    r = symsat((d (x) (c, s_) + 2^14) >> 15), (c, s_) = the Q15 sine
 *             table's (lut[(i + 1024) & 4095], lut[i]), i = ((ro_theta[s] + 2^19)
 *             >> 20) & 4095; (x), symsat, >> as in the DDS (oracle/dds_ref.c)
 *   mix       P = r conj(lo): P_I = r_I lo_I + r_Q lo_Q, P_Q = r_Q lo_I - r_I lo_Q
 *             (int32 each); S = the sum of P over the window (int64)
 *   scale     T = (S + 2^(h-1)) >> h, h = 15 + log2(spc_lo);
 *             sig = (T ro_gain[s] + 2^15) >> 16, saturated to int32 -- a
 *             full-scale LO (amp 0xFFFF, envelope 32767) and a flat-top drive
 *             give ~ amp_eff / 2 per clock, the closed form's unit
 *   noise, accumulator and outcome exactly as the DEMOD model's: z_I, z_Q the
 *             Hadamard pairs of the halves of Philox words 1, 2; acc = sig +
 *             ((z ro_sigma) >> 16); x = (acc_I axis_I + acc_Q axis_Q) >> 15;
 *             outcome = x > ro_thr.  No meas_valid: timing is the interpreter's.
 *
 * From cfg: seed, p1_threshold, meas_elem, cores_per_shot (the bound of
 * pairs->core), ro_cpw, ro_delay, ro_theta, ro_gain, ro_sigma, ro_axis, ro_thr;
 * meas_model need not be DEMOD.  The dpemu_demod_pairs arrays are HOST memory
 * (n_pairs entries each); summary / events / iq_drv / iq_lo / acc / result are
 * device pointers; iq_drv and iq_lo may be one buffer or the outputs of two
 * dpemu_dds calls with different n_samples.  n_samples_lo must be a nonzero
 * multiple of 4 (as dpemu_dds rows are) and iq_lo 16-byte aligned; event_cap
 * <= 1024; meas_cap 1..32.  result[pair] = {count = min(readouts, meas_cap),
 * outcome of readout m in bit m}; acc slots m >= count are written as zero.
 */
typedef struct dpemu_demod_pairs {
    uint32_t n_pairs, n_lanes, event_cap, meas_cap;
    uint32_t n_samples_drv, n_samples_lo;   /* row lengths of iq_drv / iq_lo */
    const uint32_t *lane, *core;            /* the pair's lane and core (< cores_per_shot) */
    const uint64_t *shot;                   /* global shot index */
    const uint32_t *drv_row, *lo_row;       /* rows of iq_drv / iq_lo */
    const uint32_t *spc_drv, *spc_lo;       /* samples per clock of the two rows, 1..16 */
} dpemu_demod_pairs;

int dpemu_demod_iq(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                   const uint32_t *summary, const uint32_t *events, const uint32_t *iq_drv,
                   const uint32_t *iq_lo, int32_t *acc /* [meas_cap][n_pairs][2] */,
                   uint32_t *result /* [n_pairs][2]: count, outcome bits */, void *stream);

/*
 * Multiplexed readout (ABI 8, additive): the rdrv returns of all qubits on a
 * readout line sum onto one feedline, and one ADC stream feeds every core's
 * rdlo demodulator -- where dpemu_demod_iq above gives every pair a private
 * ADC.  A feedline is a set of 1..DPEMU_FEEDLINE_MAX pairs of a
 * dpemu_demod_pairs table: line l holds pairs member[line_first[l] ..
 * line_first[l + 1]) (CSR offsets, line_first[0] = 0).  All members of a line
 * have the same spc_drv and spc_lo; a pair belongs to at most one line.
 *
 * dpemu_feedline_adc writes adc[n_lines][n_samples_lo], one word {I16 low, Q16
 * high} per LO-rate sample.  For LO sample j = n spc_lo + k of line l and
 * each member p:
 *   d_p     the drive sample dpemu_demod_iq's "ADC" rule picks: row drv_row[p],
 *           index (n - ro_delay) spc_drv + k (spc_drv / spc_lo), or 0 when
 *           n < ro_delay or the index is >= n_samples_drv
 *   m_p(n)  max(#{kept readouts of p's lane with t_lo <= n}, 1) - 1; the kept
 *           readouts are dpemu_demod_iq's: the meas_elem strobes among the
 *           lane's first min(n_events, event_cap) events, the first meas_cap
 *           of them (a lane without one uses draw 0 throughout)
 *   s_p     the DEMOD state draw of (seed, shot_p, core_p, m_p(n))
 *   r_p     symsat((d_p (x) (c, s_) + 2^14) >> 15), (c, s_) from ro_theta[s_p]
 *           exactly as in dpemu_demod_iq
 *   g_p     (r_p ro_gain[s_p] + 2^15) >> 16 per component (floor shift;
 *           ro_gain <= 65536, more is DPEMU_E_INVALID)
 *   adc     clamp(sum_p g_p, -32767, 32767) per component: the int32 sum
 *           saturates -- the converter clips, symmetrically
 *
 * dpemu_demod_feedline demodulates the shared stream.  For pair p of line l
 * and kept readout m:
 *   window, LO samples   those of dpemu_demod_iq
 *   mix     P = adc[l][j] conj(lo_p[j]); S = the sum of P over the window (int64).
 *           Exact for every int16 half of both words: the trace may be a
 *           caller's (a recorded one, say) and hold -32768, as an LO row may
 *           (P_I = 2^31 at four halves of -32768 does not wrap)
 *   scale   T = (S + 2^(h-1)) >> h, h = 15 + log2(spc_lo); sig = T saturated
 *           to int32 (the gain is already in the ADC)
 *   noise, acc, the discriminator, the acc / result layouts and the zeroed
 *           unused slots exactly as dpemu_demod_iq's
 * Every pair of the table must be in a line (DPEMU_E_INVALID otherwise).
 *
 * Integer arithmetic only: the result is the same for every grid.  With one
 * member per line, ro_gain = {65536, 65536} and no lane whose readout window
 * reaches its next readout strobe (the state of the return switches there),
 * acc and result equal dpemu_demod_iq's bit for bit.
 *
 * From cfg: what dpemu_demod_iq reads.  The dpemu_feedlines arrays are HOST
 * memory; summary / events / iq_drv / adc / iq_lo / acc / result are device
 * pointers.  DPEMU_E_INVALID: a NULL argument; n_lines = 0; a line that is
 * empty or has more than DPEMU_FEEDLINE_MAX members; a member >= n_pairs; a
 * pair in two lines; spc_drv or spc_lo differing within a line; and
 * dpemu_demod_iq's conditions -- n_samples_lo a nonzero multiple of 4, adc and
 * iq_lo 16-byte aligned, event_cap <= 1024, meas_cap 1..32.
 */
#define DPEMU_FEEDLINE_MAX 16
typedef struct dpemu_feedlines {           /* arrays are HOST memory */
    uint32_t n_lines;
    const uint32_t *line_first;            /* [n_lines + 1] CSR offsets into member */
    const uint32_t *member;                /* [line_first[n_lines]] pair indices */
} dpemu_feedlines;

int dpemu_feedline_adc(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                       const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                       const uint32_t *iq_drv, uint32_t *adc /* [n_lines][n_samples_lo] */, void *stream);

int dpemu_demod_feedline(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                         const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                         const uint32_t *adc /* [n_lines][n_samples_lo] */, const uint32_t *iq_lo,
                         int32_t *acc /* [meas_cap][n_pairs][2] */,
                         uint32_t *result /* [n_pairs][2]: count, outcome bits */, void *stream);

/*
 * Resonator response and converter noise (ABI 8, additive): dpemu_feedline_adc
 * with a per-member, state-dependent one-pole resonator between the drive and
 * the line, and a per-sample noise term before the converter clips.  This
 * comment is the normative definition.  The output is an ADC trace in
 * dpemu_feedline_adc's layout: dpemu_demod_feedline and dpemu_iq_stats consume
 * it unchanged.
 *
 * Pairs, lines, kept readouts, d_p, m_p(n) and s_p are exactly
 * dpemu_feedline_adc's.  For member p of line l, walk j = 0 .. n_samples_lo - 1
 * in order with y = (0, 0) before sample 0; (a, c) = coef[p][s_p(n)],
 * n = j >> log2 spc_lo:
 *   resonator  with x = d_p[j] (the int16 I, Q):
 *              y_I' = x_I + ((a_re y_I - a_im y_Q + 2^29) >> 30)
 *              y_Q' = x_Q + ((a_re y_Q + a_im y_I + 2^29) >> 30)
 *              both from the old y, int64 products, arithmetic (floor) shift.
 *              The state switches the coefficients at the strobe; y carries over.
 *   return     from the new y, per component a 16-bit signal as r_p is:
 *              g_I = clamp((c_re y_I - c_im y_Q + 2^29) >> 30, -32767, 32767)
 *              g_Q = clamp((c_re y_Q + c_im y_I + 2^29) >> 30, -32767, 32767)
 *              ro_theta and ro_gain are not read: the coupling takes their
 *              place, per pair and state
 *   noise      (adc_sigma != 0) r = Philox of (seed, shot of the line's first
 *              member, 0x80000000 | core of the line's first member, j) -- the
 *              high bit keeps the counters apart from every state and
 *              readout-noise draw; z_I, z_Q the Hadamard pairs of the 16-bit
 *              halves of words 1, 2 exactly as the DEMOD noise forms them;
 *              nu = (z adc_sigma) >> 16 per component.  It depends on the
 *              global shot, not on the line's index in the table: a sharded or
 *              re-batched run reproduces it
 *   adc        adc[l][j] = clamp(sum_p g_p + nu, -32767, 32767) per component,
 *              words {I16 low, Q16 high}
 *
 * DPEMU_E_INVALID, before any launch: everything dpemu_feedline_adc refuses
 * except its ro_gain bound; res or coef NULL; a pole with a_re^2 + a_im^2 >
 * (2^30 - 2^18)^2; a coupling component beyond +-2^30.  The pole bound |a| <=
 * 1 - 2^-12 keeps |y| <= (46341 + 1) 4096 < 2^28 (|x| <= 46341, each step's
 * rounding adds at most 1): y is an int32 that cannot overflow and every
 * product sum stays below 2^60.
 *
 * With pole (0, 0) for every pair and state, coupling (lut[(i + 1024) & 4095]
 * << 15, lut[i] << 15), i from ro_theta[s] as dpemu_feedline_adc computes it,
 * and adc_sigma = 0 the trace equals dpemu_feedline_adc's at ro_gain = {65536,
 * 65536} bit for bit: (lut 2^15 x + 2^29) >> 30 = (lut x + 2^14) >> 15.
 */
typedef struct dpemu_resonators {      /* arrays are HOST memory */
    const int32_t *coef;   /* [n_pairs][2 states][4] = pole_re, pole_im, coup_re, coup_im, Q30 */
    uint32_t adc_sigma;    /* per-sample converter noise scale; 0: none */
} dpemu_resonators;

int dpemu_feedline_adc_res(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                           const dpemu_feedlines *lines, const dpemu_resonators *res,
                           const uint32_t *summary, const uint32_t *events,
                           const uint32_t *iq_drv, uint32_t *adc /* [n_lines][n_samples_lo] */, void *stream);

/*
 * Averaged readout traces (ABI 8, additive): the time-resolved baseband
 * return of every (slot, core, prepared state) class, binned in clocks from
 * each readout's strobe -- the sums from which a host derives mean traces,
 * looks at the ring-up and builds matched-filter integration weights
 * (distributed_processor_amd/readout.py ReadoutTraces).  This comment is the
 * normative definition.
 *
 * Pairs, lines, kept readouts, their count, the window, the LO samples (with
 * the clip to n_samples_lo) and the state draw s (Philox word 0 of (seed,
 * global shot, core, m) against p1_threshold[core]) are exactly
 * dpemu_demod_feedline's.  For pair p of line l, kept readout m with its
 * strobe at t_lo, and every LO sample j = n spc_lo + k inside the window:
 *   product  P = adc[l][j] conj(lo_p[j]): dpemu_demod_feedline's "mix", int32
 *            components, exact for every int16 half of both words (-32768
 *            included; P_I reaches 2^31 and does not wrap)
 *   bin      b = (n - t_lo) / bin_clocks (floor); samples with b >= n_bins are
 *            dropped
 *   class    (by_slot ? m : 0, core_p, s)
 *   words of a class and bin (int64 each):
 *      0 readouts with at least one sample in the bin
 *      1 samples summed        2 sum P_I        3 sum P_Q
 *   traces   [S][C][2][n_bins][DPEMU_TRACE_WORDS], S = by_slot ? meas_cap : 1,
 *            C = cfg->cores_per_shot: ASSIGNED (the library zeroes it before
 *            the launch; the caller need not)
 *
 * No scaling, no noise and no discriminator: ro_sigma, ro_axis and ro_thr are
 * not read.  Integer arithmetic and integer atomics only: the result is the
 * same for every grid and schedule.  The mean baseband sample of a bin is
 * (w2 + i w3) / w1; the sum of (w2, w3) over the bins of one readout's window
 * is dpemu_demod_feedline's S.
 *
 * The dpemu_trace_bins struct is HOST memory; summary / events / adc / iq_lo /
 * traces are device pointers.  DPEMU_E_INVALID, before any launch: everything
 * dpemu_demod_feedline refuses; bins or traces NULL; n_bins 0 or above
 * DPEMU_TRACE_BINS_MAX; bin_clocks 0; by_slot > 1; traces not 8-byte aligned;
 * n_pairs * meas_cap * bin_clocks * 16 > 2^31.  That bound keeps every sum
 * below 2^62: a (class, bin) takes at most bin_clocks spc_lo <= 16 bin_clocks
 * samples of each of at most n_pairs meas_cap readouts, <= 2^31 samples, each
 * component at most 2^31 in magnitude.
 */
#define DPEMU_TRACE_WORDS 4
#define DPEMU_TRACE_BINS_MAX 4096
typedef struct dpemu_trace_bins {
    uint32_t n_bins;      /* 1..DPEMU_TRACE_BINS_MAX */
    uint32_t bin_clocks;  /* clocks per bin, >= 1 */
    uint32_t by_slot;     /* 0: one class set over all readouts; 1: one per slot m */
} dpemu_trace_bins;

int dpemu_feedline_traces(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                          const dpemu_feedlines *lines, const dpemu_trace_bins *bins,
                          const uint32_t *summary, const uint32_t *events,
                          const uint32_t *adc /* [n_lines][n_samples_lo] */, const uint32_t *iq_lo,
                          int64_t *traces /* [S][C][2][n_bins][DPEMU_TRACE_WORDS] */, void *stream);

/*
 * Readout IQ statistics (ABI 8, additive): per-class sums of an accumulator
 * buffer -- dpemu_outputs.acc of a DEMOD run, or the acc of dpemu_demod_iq --
 * from which a host derives centroids, covariances, a confusion matrix and a
 * fitted discriminator (distributed_processor_amd/readout.py).
 *
 *   readouts  (col, m) with m < min(counts[col * count_stride], meas_cap);
 *             {I, Q} = acc[m][col]
 *   state     s = (thr_p1 == 0xFFFFFFFF) || Philox word 0 of (cfg->seed, shot,
 *             core, m) < thr_p1, thr_p1 = cfg->p1_threshold[core]: the draw of
 *             the DEMOD model and of dpemu_demod_iq
 *   class     (by_slot ? m : 0, core, s)
 *   outcome   o = ((int64) I axis_I + (int64) Q axis_Q) >> 15 > thr[core], axis_I /
 *             axis_Q the int16 halves (low / high) of the core's axis word
 *   limbs     a_X = X >> 16 (arithmetic), b_X = X & 0xFFFF: X = 65536 a_X + b_X,
 *             a_X in [-2^15, 2^15), b_X in [0, 2^16)
 *   words of a class (int64 each):
 *      0 n            1 n with o = 1    2 sum I          3 sum Q
 *      4 sum a_I^2    5 sum a_I b_I     6 sum b_I^2
 *      7 sum a_Q^2    8 sum a_Q b_Q     9 sum b_Q^2
 *     10 sum a_I a_Q 11 sum (a_I b_Q + b_I a_Q)          12 sum b_I b_Q
 *     13..15 zero
 *     so sum I^2 = 2^32 w4 + 2^17 w5 + w6, sum Q^2 = 2^32 w7 + 2^17 w8 + w9,
 *     sum I Q = 2^32 w10 + 2^16 w11 + w12.  Every per-readout term is below 2^32
 *     in magnitude and n_cols * meas_cap <= 2^31 (more: DPEMU_E_INVALID), so no
 *     sum can overflow int64.
 *   bits[col] the outcome o of readout m in bit m, zero at and above the count
 *   stats     [S][C][2][DPEMU_IQ_STAT_WORDS], S = by_slot ? meas_cap : 1, C =
 *             cfg->cores_per_shot: ASSIGNED (the caller need not zero it);
 *             n_cols = 0 writes all zeros
 *
 * Integer arithmetic throughout: the result is the same for every grid and
 * schedule.  From cfg: seed, p1_threshold, cores_per_shot, and -- where cols
 * gives none -- ro_axis, ro_thr and, for the run layout, lane_order.  The
 * dpemu_iq_columns arrays are HOST memory; acc / counts / stats / bits are
 * device pointers (both 8-byte aligned; acc and counts may be NULL when n_cols
 * is 0).  DPEMU_E_INVALID: a NULL argument, meas_cap outside 1..32, by_slot > 1,
 * count_stride 0, only one of core / shot, a core >= cores_per_shot, a run
 * layout whose n_cols is no multiple of cores_per_shot.
 */
#define DPEMU_IQ_STAT_WORDS 16
typedef struct dpemu_iq_columns {      /* arrays are HOST memory */
    uint32_t n_cols;        /* columns of acc: lanes of a dpemu_run, or pairs of a dpemu_demod_iq */
    uint32_t meas_cap;      /* slots (rows) of acc, 1..32 */
    uint32_t by_slot;       /* 0: one class set over all readouts; 1: one per slot m */
    uint32_t count_stride;  /* counts[col * count_stride] = readouts of the column (clipped to meas_cap) */
    const uint32_t *core;   /* [n_cols] or NULL */
    const uint64_t *shot;   /* [n_cols] global shot, or NULL.  Both NULL: the run layout --
                               (shot, core) of column L from cfg->lane_order, cores_per_shot,
                               shot_begin and n_cols / C shots (n_cols % C == 0) */
    uint64_t shot_begin;
    const uint32_t *axis;   /* [cores_per_shot] Q15 axis words, or NULL = cfg->ro_axis */
    const int32_t  *thr;    /* [cores_per_shot] per-core thresholds, or NULL = cfg->ro_thr for all */
} dpemu_iq_columns;

int dpemu_iq_stats(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_iq_columns *cols,
                   const int32_t *acc      /* device [meas_cap][n_cols][2] */,
                   const uint32_t *counts  /* device: summary + 5 with stride 8, or result with stride 2 */,
                   int64_t *stats          /* device [S][C][2][DPEMU_IQ_STAT_WORDS], S = by_slot ? meas_cap : 1 */,
                   uint32_t *bits          /* device [n_cols], nullable */, void *stream);

/*
 * Qubit state from the drive pulses (ABI 8, additive): for every (shot, qubit
 * register) a one- or two-qubit state vector evolved through the gates the
 * drive strobes of a run stand for, its final populations and a sampled
 * outcome.  Gates come from a host-supplied dictionary of calibrated pulses;
 * the strobe's phase word (and the drive detuning) rotates the gate's axis.
 * This comment is the normative definition (CPU restatement tests/qsim_ref.py).
 * Integer arithmetic only (Q30 amplitudes, int64 products): the result is the
 * same for every grid.
 *
 *   registers  register r holds core reg_core[2r] (the "first" core) and
 *              reg_core[2r + 1] (the "second"; 0xFFFFFFFF: a one-qubit register).
 *              Row of (register r, shot) = r * n_shots + (shot - shot_begin), in
 *              pops and result alike
 *   lanes      the lane of (shot, core) is the run layout's: cfg->lane_order,
 *              cores_per_shot C and n_shots as dpemu_iq_stats reads them
 *              (core * n_shots + (shot - shot_begin), or (shot - shot_begin) * C +
 *              core)
 *   state      4 amplitudes x[j], each {re, im} int32 in Q30; j = 2 b(first core)
 *              + b(second core): the first core is the first Kronecker factor.
 *              Start: x[0] = (2^30, 0), the rest 0.  A one-qubit register uses
 *              j in {0, 2}: the absent qubit stays 0
 *   events     per lane the first min(n_events, event_cap) records (summary w2);
 *              among them the drive strobes are those of kind 0 with cfg & 3 ==
 *              drv_elem, every other record is skipped.  The drive strobes of
 *              the two lanes, each in record order, are merged two-way: while
 *              both lanes have one left, the first core's next is taken when
 *              t_first <= t_second (unsigned), else the second core's; then the
 *              rest of the other lane.  k = the taken record's slot in its lane
 *   lookup     the dictionary entry whose core is the emitting core and whose
 *              (freq, env, amp) equal the record's (w2 >> 17, w1 & 0xFFFFFF,
 *              w3 & 0xFFFF).  None: n_unmatched++, no gate, no error draw.  Else
 *              n_gates++ and:
 *   phase      phi = ((w2 & 0x1FFFF) + ((detune[c] * t) >> 15)) & 0x1FFFF, the
 *              product of the two uint32 in 64 bits, c the emitting core for kind
 *              0 and the TARGET core for kind 1 (detune NULL: all 0);
 *              w = cmulr(coarse[phi >> 8], fine[phi & 255]) = e^(2 pi i phi / 2^17)
 *              in Q30.  The tables (dpemu_qsim_phase_lut) are lrint(2^30 cos),
 *              lrint(2^30 sin) of 2 pi i / 512 (coarse, 512 entries) and of
 *              2 pi i / 2^17 (fine, 256 entries), with the four quarter-turn
 *              coarse entries exactly (+-2^30, 0) / (0, +-2^30) and fine[0] =
 *              (2^30, 0)
 *   cmulr      cmulr(p, x) = {(p_re x_re - p_im x_im + 2^29) >> 30,
 *                             (p_re x_im + p_im x_re + 2^29) >> 30}: int64
 *              products, summed before the one arithmetic (floor) shift
 *   gate       U(phi) = Rz(phi) M Rz(-phi): with M = [[a, b], [c, d]],
 *              b' = cmulr(b, conj w), c' = cmulr(c, w) (not clamped: matrix
 *              components are within +-2^30 and |w| <= 2^30 + 2, so they fit
 *              int32).  On an amplitude pair (x0, x1) of the acted qubit (x0 its
 *              bit 0, x1 its bit 1), per component:
 *                y0 = clamp(cmulr(a, x0) + cmulr(b', x1))
 *                y1 = clamp(cmulr(c', x0) + cmulr(d, x1))
 *              clamp to +-(2^31 - 1) of the int64 sum.  It never acts for
 *              near-unitary entries; it only makes every input defined.
 *              kind 0: M = m[0] on both pairs of the emitting core's qubit.
 *              kind 1 (the emitting core is the first core, the control; the
 *              second core is the target): m[0] on the target pair with control
 *              bit 0 (x[0], x[1]), m[1] on the pair with control bit 1 (x[2],
 *              x[3]), both with the same w
 *   error      (err_thr != 0) r = Philox4x32-10 of (seed, shot, 0x40000000 |
 *              emitting core, k): the philox3 of the state draws, on counters
 *              apart from theirs (core < 64) and from the ADC noise (0x80000000 |).
 *              If word 0 < err_thr: n_errors++ and, after the gate, a Pauli --
 *              kind 0: code 1 + mulhi(word 1, 3) on the emitting core's qubit;
 *              kind 1: idx = 1 + mulhi(word 1, 15), code idx >> 2 on the control
 *              and idx & 3 on the target (mulhi = the high 32 bits of the 64-bit
 *              product).  Codes: 0 I; 1 X: (y0, y1) = (x1, x0); 2 Y: (y0, y1) =
 *              (-i x1, i x0), i.e. y0 = {x1_im, -x1_re}, y1 = {-x0_im, x0_re};
 *              3 Z: x1 = -x1.  Exact: no rounding
 *   pops       pops[j] = re^2 + im^2 of x[j] (uint64, < 2^63)
 *   sample     T = the sum of pops (uint64, wraps); u = word 0 of Philox (seed,
 *              shot, 0x20000000 | first core, 0); v = floor(u T / 2^32) = u T_hi +
 *              ((u T_lo) >> 32), exact (T_hi, T_lo the 32-bit halves of T); j =
 *              how many of the running sums pops[0], pops[0] + pops[1], pops[0] +
 *              pops[1] + pops[2] (uint64, wrapping) are <= v
 *   result     {outcome: bit 0 = the first core's bit = j >> 1, bit 1 = the second
 *              core's = j & 1; n_gates; n_unmatched; (n_errors & 0xFFFF) | (a lane
 *              of the register had n_events > event_cap ? 1 << 31 : 0)}: the
 *              low half of word 3 counts the errors modulo 2^16, the bits
 *              between it and bit 31 are zero
 *
 * Out of scope of dpemu_qsim: readout strobes neither collapse nor reset the
 * state (dpemu_qsim_meas below measures at them, and its states feed the
 * interpreter's measurement bits through dpemu_run_states; dpemu_run's own stay
 * the p1_threshold draws); a pulse acts instantaneously at its strobe.
 *
 * From cfg: seed, cores_per_shot, lane_order.  The dpemu_qsim_args arrays are HOST
 * memory; summary / events / pops / result are device pointers (pops 8-byte,
 * events and result 16-byte aligned).  DPEMU_E_INVALID, before any launch: a NULL argument
 * (detune may be NULL); n_regs 0; a core >= cores_per_shot or in two registers
 * (or twice in one); more than DPEMU_QSIM_GATES_MAX entries for a core, or two
 * entries with one key; kind > 1; kind 1 on a core that is the second of its
 * register or in a one-qubit register; a gate whose core is in no register; a
 * matrix component beyond +-2^30; drv_elem > 3; event_cap >
 * DPEMU_MAX_EVENT_CAP; n_lanes != n_shots * C; n_regs * n_shots > 2^31.
 * n_shots 0 returns DPEMU_OK and launches nothing.
 */
#define DPEMU_QSIM_GATES_MAX 8            /* dictionary entries per core */
#define DPEMU_QSIM_LUT_COARSE 512
#define DPEMU_QSIM_LUT_FINE 256
typedef struct dpemu_qsim_gate {
    uint32_t core;                        /* emitting core */
    uint32_t freq, env, amp;              /* key: event w2 >> 17, w1 & 0xFFFFFF, w3 & 0xFFFF */
    uint32_t kind;                        /* 0: acts on the core's own qubit (m[0]); 1: controlled -- own qubit
                                             is the control, the register's other qubit the target: m[0] on the
                                             target when control = 0, m[1] when control = 1 */
    uint32_t err_thr;                     /* P(Pauli error after this gate) = err_thr / 2^32; 0 none */
    int32_t  m[2][8];                     /* 2x2 complex Q30, {a_re,a_im,b_re,b_im,c_re,c_im,d_re,d_im} = [[a,b],[c,d]] */
} dpemu_qsim_gate;
typedef struct dpemu_qsim_args {          /* arrays are HOST memory */
    uint32_t n_regs; const uint32_t *reg_core;   /* [n_regs][2]; second = 0xFFFFFFFF: a one-qubit register */
    uint32_t n_gates; const dpemu_qsim_gate *gates;
    uint32_t drv_elem;                    /* strobes with cfg & 3 == drv_elem are drive pulses */
    const uint32_t *detune;               /* [cores_per_shot] turns per clock, Q32, or NULL = 0 */
    uint32_t n_lanes, event_cap; uint64_t shot_begin, n_shots;   /* of the dpemu_run that wrote summary / events */
} dpemu_qsim_args;
int dpemu_qsim(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_qsim_args *qs, const uint32_t *summary,
               const uint32_t *events, uint64_t *pops /* [n_regs][n_shots][4] */,
               uint32_t *result /* [n_regs][n_shots][4] */, void *stream);
/* the Q30 {cos, sin} tables of the phase rule: 512 coarse entries, then 256 fine */
int dpemu_qsim_phase_lut(int32_t *out /* [768][2] */);

/*
 * Projective readout in the state simulation (ABI 8, additive): dpemu_qsim
 * word for word, except that a readout strobe measures the emitting core's
 * qubit -- it samples an outcome, collapses the state and renormalises -- and
 * that the post-measurement state bit of every readout is written to `states`.
 * This comment is the normative definition (CPU restatement
 * tests/qsim_meas_ref.py).  Integer arithmetic only; nothing is rounded.
 *
 *   records    per lane the kept records are the drive strobes (dpemu_qsim's)
 *              and the readout strobes: kind 0 with cfg & 3 == cfg->meas_elem,
 *              both among the lane's first min(n_events, event_cap) records, in
 *              record order.  The two-way merge across a register's lanes and
 *              its tie rule (t_first <= t_second takes the first core's) are
 *              dpemu_qsim's, over both kinds of record.  k, the record slot of
 *              the error draws, is unchanged: on a stream without readout
 *              strobes pops and result equal dpemu_qsim's bit for bit
 *   readout m  of a lane, m = that lane's readout strobes taken so far:
 *              P[j] = re^2 + im^2 of x[j] (uint64); T = the sum of P, wrapping
 *              as in the sample rule; A = the sum of the P[j] whose bit of this
 *              core's qubit is 1 -- the first core: P[2] + P[3], the second:
 *              P[1] + P[3]; u = word 0 of Philox (seed, shot, 0x10000000 | core,
 *              m): core < 64, so a counter range apart from the state, error
 *              (0x40000000 |), sample (0x20000000 |) and ADC-noise (0x80000000 |)
 *              draws; v = floor(u T / 2^32) by the sample rule's two-half
 *              formula; outcome b = (T - A <= v) (uint64, wrapping): P(1) = A / T
 *   collapse   every x[j] whose bit of this qubit differs from b becomes (0, 0)
 *   shift      T' = the sum of the remaining pops; s = T' == 0 ? 0 :
 *              max(0, (59 - msb(T')) >> 1), msb the index of the highest set
 *              bit; every component of every amplitude is shifted left by s.
 *              T' 4^s lies in [2^58, 2^60) whenever T' < 2^58, no component
 *              exceeds 2^30 afterwards (the gate rule's bounds hold), and a
 *              power of two rounds nothing.  The sample rule normalises by T:
 *              the state need not be of unit norm
 *   states     if m < 32, bit m of states[lane] is b; readouts with m >= 32
 *              still measure and collapse but are not recorded.  No gate
 *              lookup and no error draw happens at a readout strobe; n_gates
 *              and n_unmatched do not count it.  states[lane] is ASSIGNED: the
 *              library zeroes the n_lanes words on the call's stream before
 *              the kernel runs; lanes of cores in no register, and all bits at
 *              or above a lane's readout count, read 0
 *   pops, result  as dpemu_qsim's, from the final (collapsed, shifted) state
 *
 * A measurement acts instantly at the readout strobe's t -- the instant at
 * which dpemu_feedline_adc switches a member's state.  dpemu_run's own
 * measurement bits and branches stay the p1_threshold draws; dpemu_run_states
 * takes this call's `states` in their place, and alternating the two calls
 * until the buffer reproduces itself simulates a measurement-conditioned
 * program along the qubit's path (DESIGN.md §2 "Co-simulation").  The qubit
 * is ideal between its strobes; dpemu_qsim_decay below lets it relax and dephase.
 *
 * `states` is a device pointer to n_lanes words.  DPEMU_E_INVALID, before any
 * launch: everything dpemu_qsim refuses; states NULL; cfg->meas_elem > 3;
 * cfg->meas_elem == qs->drv_elem.  n_shots 0 returns DPEMU_OK and launches
 * nothing (states is not touched).
 */
int dpemu_qsim_meas(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_qsim_args *qs,
                    const uint32_t *summary, const uint32_t *events, uint64_t *pops /* [n_regs][n_shots][4] */,
                    uint32_t *result /* [n_regs][n_shots][4] */, uint32_t *states /* device [qs->n_lanes] */,
                    void *stream);

/*
 * Decoherence between pulses, T1 / T2 (ABI 8, additive): dpemu_qsim (states ==
 * NULL) or dpemu_qsim_meas (states != NULL, its output) word for word, plus one
 * rule: before a gate or a measurement acts on a qubit, that qubit is first
 * ADVANCED over the clocks since it was last advanced.  An advance is one
 * quantum-trajectory step: amplitude damping as the no-jump decay of the |1>
 * amplitudes plus a sampled jump to |0>, pure dephasing as a sampled Z flip.
 * Averaged over shots the rows reproduce the Lindblad channel with 1 / T2 =
 * 1 / (2 T1) + 1 / Tphi.  This comment is the normative definition (CPU
 * restatement tests/qsim_decay_ref.py).  Integer arithmetic and counter-based
 * draws only: the result is the same for every grid and every batching.
 *
 *   tables     damp[c][i] (Q30) is the |1> AMPLITUDE factor of core c's qubit
 *              over 2^i clocks, e^(-2^i / (2 T1)); deph[c][i] (Q30) the
 *              pure-dephasing coherence factor over 2^i clocks, e^(-2^i / Tphi).
 *              2^30 = no decay over that span
 *   span       for a span dt (uint32) and a table tab[32]: F = 2^30; for i = 0 ..
 *              31 ascending, if bit i of dt is set, F = (F tab[i] + 2^29) >> 30
 *              (a 64-bit product).  G from damp, E from deph, both in [0, 2^30]
 *   clock      each qubit of a register carries tl, 0 at the start.  "Advance to
 *              t": if t > tl (unsigned), dt = t - tl and tl = t, and the two steps
 *              below run with G and E of dt; otherwise nothing happens (records
 *              out of time order are defined and harmless)
 *   when       in the merged stream of the base call: a taken readout strobe
 *              (states != NULL only) advances the emitting core's qubit to the
 *              record's t, then measures.  A drive strobe whose lookup hits
 *              advances -- before the phase and gate rules -- the emitting core's
 *              qubit (kind 0), or the control (the emitting core's qubit) and then
 *              the target (kind 1).  An unmatched strobe advances nothing.  After
 *              the stream, if t_final != 0, the first core's qubit and then the
 *              second's advance to t_final, before pops and the sample
 *   draws      an advance takes one Philox (the philox3 of the other draws) on
 *              (seed, shot, tag | core, n): a qubit advanced by its own core's
 *              record: tag 0x08000000, that core, n = the record's slot k; a
 *              target advanced by the control's record: tag 0x04000000, the
 *              target core, n = the control's slot k; the final advance: tag
 *              0x02000000, that core, n = 0.  Counter ranges apart from one another
 *              and from the state (core < 64), readout (0x10000000 |), sample
 *              (0x20000000 |), error (0x40000000 |) and ADC-noise (0x80000000 |)
 *              draws
 *   pairs      the qubit's amplitude pairs (x_lo, x_hi) are (x[0], x[2]), (x[1],
 *              x[3]) for the first core's qubit and (x[0], x[1]), (x[2], x[3]) for
 *              the second's
 *   damping    only when G < 2^30.  T = the sum of pops, A = the sum of pop(x_hi)
 *              (uint64, wrapping, as in the sample rule).  y_hi = (G x_hi + 2^29)
 *              >> 30 per component (int64 product, floor shift): |y| <= |x| per
 *              component, so A' = the sum of pop(y_hi) <= A.  u = word 0 of the
 *              draw, v = floor(u T / 2^32) by the two-half formula.  Jump iff
 *              v < A - A': P(jump) = P(1) (1 - G^2).  On a jump, in both pairs,
 *              x_lo = the old x_hi and x_hi = (0, 0); otherwise x_hi = y_hi.  Then
 *              the shift of dpemu_qsim_meas on the new total T': s = T' == 0 ? 0 :
 *              max(0, (59 - msb(T')) >> 1), every component of every amplitude
 *              shifted left by s: exact, and the gate rule's bounds hold (int32
 *              arithmetic modulo 2^32, here and in the negation below: it shows
 *              only where a wrapped total lets a shift pass 2^31, which a state
 *              within the gate rule's bounds never does)
 *   dephasing  thr = (2^30 - E) << 1; if word 1 of the draw < thr, x_hi = -x_hi in
 *              both pairs (after the damping step; exact)
 *   identity   with G = 2^30 the damping step and its shift do not happen, with
 *              E = 2^30 no flip can, with dt = 0 nothing does: an implementation
 *              may skip the draw then.  With every table entry 2^30 and t_final 0,
 *              pops, result and states equal the base call's bit for bit
 *   counts     (nullable) per row the four words {jumps of the first core's
 *              qubit, flips of the first, jumps of the second, flips of the
 *              second}; a flip is counted whenever its draw passes, even after a
 *              jump.  Assigned for every row
 *
 * Unchanged from the base call: result, pops and states and their layouts,
 * n_gates / n_unmatched / n_errors, the error draws and their slot k, the merge
 * and its tie rule, the overflow bit, the zeroing of states.  Out of scope: no
 * decay during a pulse or a readout window (both act instantly), no thermal
 * excitation (the jump goes to |0> only), no correlated noise (every qubit has
 * its own draws).
 *
 * damp and deph are HOST arrays of cores_per_shot x 32 words; counts is a
 * device pointer (16-byte aligned) or NULL.  DPEMU_E_INVALID, before any launch:
 * everything the base call refuses (dpemu_qsim's list; with states != NULL
 * dpemu_qsim_meas's conditions on cfg->meas_elem); dec, damp or deph NULL; a
 * table entry above 2^30.  n_shots 0 returns DPEMU_OK and launches nothing.
 */
typedef struct dpemu_qsim_decay_args {      /* arrays are HOST memory */
    const uint32_t *damp;   /* [cores_per_shot][32] Q30: entry i = the |1> AMPLITUDE factor over 2^i clocks, e^(-2^i / (2 T1)) */
    const uint32_t *deph;   /* [cores_per_shot][32] Q30: entry i = the pure-dephasing coherence factor over 2^i clocks, e^(-2^i / Tphi) */
    uint32_t t_final;       /* != 0: every qubit is advanced to this clock before pops are taken */
} dpemu_qsim_decay_args;
int dpemu_qsim_decay(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_qsim_args *qs,
                     const dpemu_qsim_decay_args *dec, const uint32_t *summary, const uint32_t *events,
                     uint64_t *pops /* [n_regs][n_shots][4] */, uint32_t *result /* [n_regs][n_shots][4] */,
                     uint32_t *states /* NULL: dpemu_qsim's records; else dpemu_qsim_meas's, and its output */,
                     uint32_t *counts /* device [n_regs][n_shots][4], nullable */, void *stream);

/*
 * States into the readout stages (ABI 8, additive): each call is its base call
 * with one more device pointer before `stream`.  With states == NULL it is the
 * base call exactly (same code path, same bytes).  Otherwise the prepared
 * state of a readout is read from `states` wherever the base definition draws
 * it -- "the DEMOD state draw of (seed, shot_p, core_p, m)" -- and
 * p1_threshold is not read; the noise draws (Philox words 1, 2) are untouched.
 *
 *   feedline calls   states has pairs->n_lanes words; the state of pair p at
 *                    kept readout m is (states[pairs->lane[p]] >> m) & 1, a lane
 *                    without a readout uses bit 0.  dpemu_qsim_meas's buffer of
 *                    the same run is passed as it is
 *   dpemu_iq_stats_st  states has cols->n_cols words; the state of (col, m) is
 *                    (states[col] >> m) & 1.  In the run layout a column is a
 *                    lane: dpemu_qsim_meas's buffer as it is; for a pair table
 *                    the caller gathers states[pairs.lane]
 *
 * dpemu_demod_feedline reads no state (the gain is already in the ADC) and
 * dpemu_demod_iq keeps its draw (a one-member feedline serves that case):
 * neither has a variant.  dpemu_last_kernel and the timing pair are the base
 * call's.
 */
int dpemu_feedline_adc_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                          const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                          const uint32_t *iq_drv, uint32_t *adc /* [n_lines][n_samples_lo] */,
                          const uint32_t *states /* device [pairs->n_lanes], nullable */, void *stream);
int dpemu_feedline_adc_res_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                              const dpemu_feedlines *lines, const dpemu_resonators *res,
                              const uint32_t *summary, const uint32_t *events, const uint32_t *iq_drv,
                              uint32_t *adc /* [n_lines][n_samples_lo] */,
                              const uint32_t *states /* device [pairs->n_lanes], nullable */, void *stream);
int dpemu_feedline_traces_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                             const dpemu_feedlines *lines, const dpemu_trace_bins *bins,
                             const uint32_t *summary, const uint32_t *events,
                             const uint32_t *adc /* [n_lines][n_samples_lo] */, const uint32_t *iq_lo,
                             int64_t *traces /* [S][C][2][n_bins][DPEMU_TRACE_WORDS] */,
                             const uint32_t *states /* device [pairs->n_lanes], nullable */, void *stream);
int dpemu_iq_stats_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_iq_columns *cols,
                      const int32_t *acc, const uint32_t *counts, int64_t *stats, uint32_t *bits /* nullable */,
                      const uint32_t *states /* device [n_cols], nullable */, void *stream);

/*
 * Measurement.  While kernel timing is on, dpemu_run, dpemu_run_states, dpemu_dds,
 * dpemu_demod_iq, dpemu_feedline_adc, dpemu_feedline_adc_res,
 * dpemu_demod_feedline, dpemu_feedline_traces, dpemu_iq_stats, dpemu_qsim,
 * dpemu_qsim_meas, dpemu_qsim_decay (round the kernel, not the zeroing of states) and the *_st calls
 * record a HIP event pair on the call's stream around their main kernel (the
 * interpreter / the DDS kernel / demod_iq_kernel / feedline_adc_kernel /
 * feedline_res_kernel / feedline_demod_kernel / feedline_trace_kernel /
 * iq_stats_kernel / qsim_kernel; not the histogram memset and
 * reduction, the DDS or feedline index, the outcome-bit pass or the zeroing of
 * stats or traces).
 * dpemu_kernel_times waits for the recorded pairs, writes up to max_n
 * elapsed times in ms (oldest first) to ms, *n_out = how many, and clears the
 * record.  dpemu_last_kernel names the interpreter variant the last dpemu_run
 * or dpemu_run_states
 * launched (e.g. "straight_kernel<rows,fb1>", "macro_kernel", "interp_kernel<feat=0x3>"),
 * or "demod_iq_kernel" after a dpemu_demod_iq, "feedline_adc_kernel" /
 * "feedline_demod_kernel" after the two feedline stages, "feedline_res_kernel"
 * after a dpemu_feedline_adc_res, "feedline_trace_kernel" after a
 * dpemu_feedline_traces, "iq_stats_kernel"
 * after a dpemu_iq_stats with n_cols > 0, "qsim_kernel" after a dpemu_qsim
 * and "qsim_kernel<meas>" after a dpemu_qsim_meas with n_shots > 0,
 * "qsim_kernel<decay>" / "qsim_kernel<meas,decay>" after a dpemu_qsim_decay
 * without / with states.
 */
int         dpemu_set_kernel_timing(dpemu_ctx *ctx, int enable);
int         dpemu_kernel_times(dpemu_ctx *ctx, float *ms, int max_n, int *n_out);
const char *dpemu_last_kernel(dpemu_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* DPEMU_H */
