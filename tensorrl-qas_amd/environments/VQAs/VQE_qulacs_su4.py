"""The reference's SU(4) seam (environments/VQAs/VQE_qulacs_su4.py) with the same names and argument
meaning, backed by libvqe_hip.so instead of qulacs + a dense numpy matvec.

    circ = Parametric_Circuit(n).construct_ansatz(state)       # state: (L, 6n+6, n)
    e = get_exp_val(n, circ, observable)
    e = get_energy_qulacs(angles, observable, circ, n, n_shots)

The ansatz is built from RXX / RYY / RZZ (the reference's ParametricPauliRotation([a, b], [P, P], theta))
followed by the one-qubit rotations of every layer; the circuit starts from |0..0>.  ``observable`` is a
``PauliHamiltonian`` (tensorrl_qas_amd.hamiltonian) or a dense matrix in the simulator's little-endian basis."""
from ... import circuits as _circ
from .VQE_qulacs_TN_notin_RL import _engine_for


class Parametric_Circuit:
    def __init__(self, n_qubits, noise_models=[], noise_values=[]):
        self.n_qubits = n_qubits
        self.ansatz = None
        self.angles = None

    def construct_ansatz(self, state):
        self.ansatz, self.angles = _circ.circuit_from_state_su4(state, self.n_qubits)
        self.ansatz.angles = self.angles.copy()     # the circuit handle carries its parameters
        return self.ansatz


def get_exp_val(n_qubits, circuit, op):
    eng = _engine_for(n_qubits, op, None)
    eng.set_circuit(circuit)
    return eng.energy(circuit.angles)


def get_energy_qulacs(angles, observable, circuit, n_qubits, n_shots, phys_noise=False, which_angles=[]):
    which = list(which_angles) if list(which_angles) else range(circuit.n_params)
    for i, j in enumerate(which):
        circuit.angles[j] = angles[i]
    return get_exp_val(n_qubits, circuit, observable)
