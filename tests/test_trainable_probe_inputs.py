"""CPU: the exact-probe inputs of tests/test_gpu_trainable_paths.py are what that file needs them to be — exactly representable in bf16 / fp16, some t
needing its low 16-bit part, every 64-row chunk reaching an output, and every sum of |terms| below 2^24 units, so that the GPU results must equal
fp64 under any summation order.  The constructors are index arithmetic: the same tensors on any device."""
import test_gpu_trainable_paths as P


def test_lora_probe_inputs_fit_24_bits():
    P.check_lora_probe_inputs("cpu")


def test_adapter_probe_inputs_are_exact_and_structured():
    P.check_adapter_probe_inputs("cpu")
