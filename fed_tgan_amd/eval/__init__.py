from .privacy import DevicePrivacy, PrivacyScores  # noqa: F401
