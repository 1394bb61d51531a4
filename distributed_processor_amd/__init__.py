"""MI355X-native batched emulator of the QubiC distributed processor.

Host side of the emulator: ISA encoder/decoder (``isa``), hardware-config
plugins (``hwconfig``), and the ``Emulator`` front end that runs assembled
distproc programs on hand-written CDNA4 HIP kernels through the C ABI in
``include/dpemu.h`` (interpreter, DDS synthesis ``dds``, and the demodulation
of the synthesised readout channels, ``Emulator.demodulate`` -- or, for qubits
multiplexed on a shared feedline (``FeedlineTable``), ``Emulator.feedline_adc``
and ``Emulator.demodulate_feedline``, with a per-qubit resonator response and
converter noise when given a ``ResonatorTable`` -- and the readout
statistics and discriminator fit of ``readout``: ``Emulator.iq_stats``,
``ReadoutStats``, ``Discriminator``, and the averaged traces and matched-filter
weights of ``Emulator.feedline_traces`` / ``ReadoutTraces``; and the qubit states the drive pulses
produce, ``qsim``: ``GateSet``, ``Emulator.simulate_gates`` (with ``measure=True`` a projective readout whose states the readout stages take), ``survival``, ``readout_survival``, ``fit_decay``); upstream of it, the restated compiler scheduling
stage (``schedule``) and the API-compatible assembler (``assembler``) that turn QubiC circuits
into that machine code.
"""

from . import dds, isa, hwconfig, lint, qsim, readout, schedule  # noqa: F401
from .dds import FeedlineTable, ResonatorTable  # noqa: F401
from .qsim import GateSet, fit_decay, readout_survival, state_bits, survival  # noqa: F401
from .readout import Discriminator, ReadoutStats, ReadoutTraces  # noqa: F401

__all__ = ['dds', 'isa', 'hwconfig', 'lint', 'qsim', 'readout', 'schedule', 'Discriminator', 'FeedlineTable', 'GateSet', 'ReadoutStats',
           'ReadoutTraces', 'ResonatorTable', 'fit_decay', 'readout_survival', 'state_bits', 'survival']
