"""Host side of the whole-sequence ConvLSTM scan: the C-ABI symbols, the supported range and the routing predicate of
``layer_gen.ConvLSTM`` (no device, no launch)."""
import pytest
import torch

SYMBOLS = ("snn_convlstm_seq_supported", "snn_convlstm_seq_fwd", "snn_convlstm_seq_bwd")


def test_symbols_exist_in_library_and_binding(hip_lib):
    from snn_for_object_detection_amd import _hip
    for name in SYMBOLS + ("snn_convlstm_seq_tile",):
        assert name in _hip.SIGNATURES
        assert getattr(hip_lib, name) is not None
    assert hip_lib.snn_abi_version() == 20   # symbols were only added


@pytest.mark.parametrize("Cin,Ch", [(3, 16), (20, 48), (256, 256)])
def test_supported_range_yes(hip_lib, Cin, Ch):
    from snn_for_object_detection_amd import functional as HF
    assert HF.conv_lstm_scan_covers(Cin, Ch, Cin)
    assert HF.conv_lstm_scan_covers(Cin, Ch, Cin + 9)
    assert HF.conv_lstm_scan_tile(Cin, Ch, 1) in (16, 32)


@pytest.mark.parametrize("Ch", [4, 12, 272])
def test_supported_range_no(hip_lib, Ch):
    from snn_for_object_detection_amd import functional as HF
    assert not HF.conv_lstm_scan_covers(8, Ch, 8)
    assert HF.conv_lstm_scan_tile(8, Ch, 100) == 0


def test_pixel_stride_below_channels_is_refused(hip_lib):
    from snn_for_object_detection_amd import functional as HF
    assert not HF.conv_lstm_scan_covers(20, 48, 19)
    assert not HF.conv_lstm_scan_covers(0, 16, 4) and not HF.conv_lstm_scan_covers(257, 16, 257)


def test_tile_is_a_multiple_of_the_mfma_rows(hip_lib):
    from snn_for_object_detection_amd import functional as HF
    for M in (1, 17, 8245, 1 << 22):
        for Ch in (16, 128, 144, 256):
            P = HF.conv_lstm_scan_tile(64, Ch, M)
            assert P in (16, 32) and (Ch <= 128 or P == 16)   # the backward operand tile of Ch > 128 fits LDS at P = 16 only


def test_conv_lstm_routing(hip_lib, monkeypatch):
    from snn_for_object_detection_amd import functional as HF
    from snn_for_object_detection_amd.layer_gen import ConvLSTM
    monkeypatch.setattr(HF, "USE_LSTM_SCAN", True)
    cell = ConvLSTM(20, 48)
    seq = torch.zeros(3, 2, 20, 4, 5)
    state = (torch.zeros(2, 48, 4, 5), torch.zeros(2, 48, 4, 5))
    assert cell.takes_scan(seq) and cell.takes_scan(seq, state)
    assert cell.takes_scan(torch.zeros(3, 2, 4, 5, 29)[..., 4:24].permute(0, 1, 4, 2, 3))   # channel slice, ldx = 29
    assert cell.takes_scan(seq[0], state)                               # one timestep = a sequence of one: same bits as layer-major
    assert not cell.takes_scan(seq[0, 0])
    assert not cell.takes_scan(seq.to(torch.bfloat16))                  # bf16 storage stays stepwise
    assert not cell.takes_scan(seq, (None, state[1]))
    for Ch in (4, 5, 12):                                               # the hidden sizes of the existing tests
        assert not ConvLSTM(3, Ch).takes_scan(torch.zeros(3, 2, 3, 4, 5))
    assert not ConvLSTM(20, 48, kernel_size=3).takes_scan(seq)
    monkeypatch.setattr(HF, "USE_LSTM_SCAN", False)
    assert not cell.takes_scan(seq)
    assert list(cell.state_dict()) == ["conv.weight"]
