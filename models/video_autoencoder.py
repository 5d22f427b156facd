"""`models.video_autoencoder` import surface (reference models/video_autoencoder.py) -> HIP-backed modules."""
import importlib

_impl = importlib.import_module("video-anomaly-detection_amd.video_autoencoder")
ConvLSTMCell, ConvLSTM = _impl.ConvLSTMCell, _impl.ConvLSTM
VideoEncoder, VideoDecoder, VideoAutoencoder = _impl.VideoEncoder, _impl.VideoDecoder, _impl.VideoAutoencoder
VideoState = _impl.VideoState
