"""Helper.decompress_binary_images (content/helper.py:27-34): PNG list -> list of uint8 frames
(LM_PNG_CODEC=device: decoded on the device, lecturemath_amd.png_device, and copied back)."""
from lecturemath_amd import png, png_device


class Helper:
    @staticmethod
    def decompress_binary_images(compressed_images):
        if png_device.codec() == "device" and len(compressed_images):
            w, h = png_device.png_size(compressed_images[0])
            codec = png_device.get_codec(w, h)
            return list(codec.be.to_host(png_device.decode_gray8_device(compressed_images, w, h)))
        return [png.decode_gray8(raw) for raw in compressed_images]
